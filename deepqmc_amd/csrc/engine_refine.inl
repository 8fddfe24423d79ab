// engine_refine.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip (one translation unit):
// float64 refinement of a float32 context: the twin, gather -> float64 pass -> write-back, self-calibration of the score
// threshold, the whole-batch float64 mode with hysteresis.

  int ensure_twin() {
    if (twin) return DQMC_OK;
    if (no_twin) return fail(DQMC_E_UNSUPPORTED, "the float64 twin of this context is switched off (option no_twin)");
    auto* t = new Engine<double>();
    t->st = st; t->device = device;
    dqmc_system s2 = sys;
    s2.dtype = 1;
    int rc = t->init(&s2, charges_h.data(), bufs.data(), (int)bufs.size(), ops.data(), (int)ops.size(), w64_h.data(), w64_h.size(),
                     h_itable.data(), h_itable.size());
    if (!rc && (!ecp_loc_h.empty() || !ecp_nl_h.empty()))      // the twin carries the whole ECP: its local energies include V_nl
      rc = t->set_ecp(ecp_loc_nt_h, ecp_loc_h.empty() ? nullptr : ecp_loc_h.data(), ecp_nl_L_h, ecp_nl_nt_h, ecp_nl_h.empty() ? nullptr : ecp_nl_h.data());
    if (!rc && !ph_mask_h.empty()) rc = t->set_ph(ph_grid, ph_rmax, ph_loc_h.data(), ph_l2_h.data(), ph_mask_h.data());
    for (size_t k = 0; k < twin_opts.size() && !rc; ++k) rc = t->option(twin_opts[k].first.c_str(), twin_opts[k].second);
    if (rc) { delete t; return rc; }
    t->ecp_seed = ecp_seed; t->ecp_phi = ecp_phi;      // (later ones: ecp_rotation)
    t->ws_budget = twin_full_budget ? ws_budget : ws_budget / 2;
    t->timing = timing;
    twin = t;
    return seed_twin_from_device();      // (after device updates w64_h is stale: engine_optim.inl)
  }
  // float64 results of the n walkers listed in d_flag[1..n] replace the float32 ones.  d_count != nullptr: the list
  // holds fewer than n entries -- the count is read on the device, n is the (padded) size of this pass (kernels_mcmc.hip:
  // k_refine_gather).  A probe call passes `rethreshold`: it is handed the n float64 energies on the host between the twin's
  // pass and the write-back, and only walkers whose score lies above refine_thresh as it stands after it are written back.
  template <class Rethreshold = std::nullptr_t>
  int refine_listed(const real* r, const real* R, int B, int n, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign,
                    bool skip_nl, const int32_t* d_count = nullptr, Rethreshold&& rethreshold = nullptr) {
    constexpr bool probe = !std::is_same_v<std::decay_t<Rethreshold>, std::nullptr_t>;
    const int32_t* d_list = d_flag + 1;
    const int n3 = 3 * N, nR3 = 3 * sys.n_nuc;
    Slab slab;
    const auto o_r = slab.take<double>((size_t)n * n3), o_R = slab.take<double>(nR3), o_e = slab.take<double>(n),
               o_s = slab.take<double>(6 * (size_t)n), o_g = slab.take<double>((size_t)n * n3), o_l = slab.take<double>(n);
    const auto o_sg = slab.take<int32_t>(n);
    { const int rc = d_ref.reserve(slab.bytes, st); if (rc) return rc; }
    double *r64 = o_r.in(d_ref), *R64 = o_R.in(d_ref), *e64 = o_e.in(d_ref), *s64 = o_s.in(d_ref), *g64 = o_g.in(d_ref), *l64 = o_l.in(d_ref);
    int32_t* sg64 = o_sg.in(d_ref);
    t_begin("refine", 0);
    dqmc::launch_refine_gather(st, (const float*)r, (const float*)R, d_list, d_count, n, n3, nR3, r64, R64);
    t_end();
    PassOpts t;
    t.skip_ph = (e_loc == nullptr);       // psi_grad / Langevin: the plain gradient, no pseudo-Hamiltonian seeding
    // a Hamiltonian with a non-local ECP: the twin runs the quadrature of its walkers in float64 with the rotation angles
    // of the walkers they stand for (its psi ratios carry the float64 value path's accuracy: float32 ratios alone put
    // ~1e-4 relative on E_loc of a 30-electron Psiformer)
    t.skip_nl = (e_loc == nullptr) || skip_nl;      // (deferred: ecp_mixed adds V_nl to every walker afterwards)
    t.walker_idx = d_list; t.phi_f32 = true;
    const int rc = twin->lap_refined(r64, R64, n, e64, s64, g64, l64, sg64, t);
    if (twin->last_chunks[0] > last_chunks[1]) last_chunks[1] = twin->last_chunks[0];
    if (rc) return rc;
    t_begin("refine", 0);
    if constexpr (probe) {
      // the new threshold needs the float64 energies of the sample on the host first; then only the walkers above it are
      // written back (d_score / refine_thresh at that moment)
      std::vector<double> e_h((size_t)n);
      HIP_TRY(hipMemcpyAsync(e_h.data(), e64, sizeof(double) * e_h.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      rethreshold(e_h);
    }
    dqmc::launch_refine_scatter(st, d_list, d_count, n, n, probe ? d_score.p : nullptr, refine_thresh, n3, e64, s64, g64, l64, sg64,
                                (float*)e_loc, (float*)stats, (long)B, (float*)grad, (float*)logpsi, sign);
    t_end();
    return DQMC_OK;
  }

  // error-predictor scores of the last float32 pass that flagged (host copy; walkers of that call, in order)
  int last_score_B = 0;
  int refine_scores(double* out, int n) override {
    if (sizeof(real) != 4 || !d_score || last_score_B < 1) return fail(DQMC_E_UNSUPPORTED, "no float32 pass with the error predictor has run on this context");
    if (n > last_score_B) return fail(DQMC_E_ARG, "more scores requested than the last flagged pass had walkers");
    HIP_TRY(hipMemcpyAsync(out, d_score, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DQMC_OK;
  }
  int upload_list(const std::vector<int32_t>& idx) {
    std::vector<int32_t> buf(idx.size() + 1);
    buf[0] = (int32_t)idx.size();
    std::copy(idx.begin(), idx.end(), buf.begin() + 1);
    HIP_TRY(hipMemcpyAsync(d_flag, buf.data(), sizeof(int32_t) * buf.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DQMC_OK;
  }
  // The forward-Laplacian pass of a local-energy / psi_grad / Langevin call with its bookkeeping.  A float64 context runs the
  // pass it is asked for (`opts`: a twin is told by the float32 context it serves); a float32 context decides by itself
  // (lap_f32) and, for a Hamiltonian with a non-local ECP under "ecp_mixed", splits the call: kinetic part first (float32
  // pass, flagged walkers re-run in float64 WITHOUT the quadrature), then V_nl of every walker with the precision chosen per
  // (nucleus, electron) pair.
  int lap_refined(const real* r, const real* R, int B, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign,
                  const PassOpts& opts = {}) {
    last_refined = 0;
    ++refine_counters[0];
    int rc;
    if constexpr (sizeof(real) == 8) {
      rc = pass_own(r, R, B, logpsi, sign, e_loc, stats, grad, opts);
    } else {
      const bool mixed = refine == 1 && ecp_mixed_on && ecp_n_nl > 0 && e_loc;
      rc = lap_f32(r, R, B, e_loc, stats, grad, logpsi, sign, mixed);
      if (!rc && mixed) rc = ecp_mixed((const float*)r, (const float*)R, B, (float*)e_loc, (float*)stats);
    }
    refine_counters[3] += last_refined;
    refine_info[0] = sizeof(real) == 8 ? 0 : refine; refine_info[1] = refine_thresh; refine_info[2] = probe_c; refine_info[3] = direct.calls_left;
    return rc;
  }
  // The float32 body: the pass in float32 with k_final flagging, then one of three steps -- or, in the direct mode, the
  // first of them alone.  skip_nl: the non-local ECP quadrature follows in ecp_mixed, neither pass runs it.
  int lap_f32(const real* r, const real* R, int B, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign, bool skip_nl) {
    PassOpts own;
    own.skip_nl = skip_nl;
    if (!refine) return pass_own(r, R, B, logpsi, sign, e_loc, stats, grad, own);
    int rc = d_flag.reserve((size_t)B + 1, st);
    if (!rc) rc = d_score.reserve((size_t)B, st);
    if (rc) return rc;
    // mode 1 on a system where most walkers get flagged (deep attention networks, ill-conditioned Slater matrices of a
    // random-init TransPsiformer): the float32 pass would be wasted, so the following 15 calls go to float64 directly,
    // then the float32 pass is probed again
    const bool stay = refine == 1 && direct.take_call();
    if (refine >= 2 || (stay && twin)) {
      last_score_B = 0;          // (no float32 pass, no scores)
      rc = ensure_twin();
      if (rc) return rc;
      return refine_whole(r, R, B, e_loc, stats, grad, logpsi, sign, skip_nl);
    }
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), st));
    rc = d_thresh.reserve(1, st);
    if (rc) return rc;
    if (thresh_uploaded != refine_thresh) {      // (k_final reads the threshold from here: a captured pass must follow a re-calibration)
      HIP_TRY(hipMemcpyAsync(d_thresh, &refine_thresh, sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
      thresh_uploaded = refine_thresh;
    }
    own.flag = true;
    rc = pass_own(r, R, B, logpsi, sign, e_loc, stats, grad, own);
    last_score_B = rc ? 0 : B;
    if (rc) return rc;
    const bool probe = refine == 1 && refine_probe > 0 && e_loc && (calls_since_probe < 0 || calls_since_probe + 1 >= refine_probe);
    if (calls_since_probe >= 0) ++calls_since_probe;
    int32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n > B) n = B;
    if (!probe && n <= 0) { direct.decide(0, B); return DQMC_OK; }      // (a float32 look that flags nothing leaves the direct mode: reset the hysteresis state)
    if (probe) ++refine_counters[2];
    rc = ensure_twin();
    if (rc == DQMC_E_UNSUPPORTED && refine == 1) { refine = 0; return DQMC_OK; }   // no float64 kernel set for this program: float32 stands
    if (rc) return rc;
    rc = probe ? refine_probed(r, R, B, n, e_loc, stats, grad, logpsi, sign, skip_nl)
               : refine_flagged(r, R, B, n, e_loc, stats, grad, logpsi, sign, skip_nl);
    HIP_TRY(hipGetLastError());
    return rc;
  }
  // step "direct": the whole forward-Laplacian pass in float64 (float32 stays the sampling dtype)
  int refine_whole(const real* r, const real* R, int B, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign, bool skip_nl) {
    ++refine_counters[1];
    std::vector<int32_t> iota((size_t)B);
    for (int k = 0; k < B; ++k) iota[k] = k;
    int rc = upload_list(iota);
    if (!rc) rc = refine_listed(r, R, B, B, e_loc, stats, grad, logpsi, sign, skip_nl);
    if (!rc) last_refined = B;
    return rc;
  }
  // step "flagged": the n > 0 walkers k_final listed in d_flag
  int refine_flagged(const real* r, const real* R, int B, int n, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign, bool skip_nl) {
    // most of the batch is beyond float32: this call and the next 15 evaluate everything in float64
    if (refine == 1 && direct.decide(n, B)) return refine_whole(r, R, B, e_loc, stats, grad, logpsi, sign, skip_nl);
    // the twin's pass replays a captured graph per batch size: round the count up to a multiple of 64 (the surplus rows
    // re-evaluate the first flagged walker and are not written back: k_refine_gather / scatter read the count on the
    // device), so that a handful of sizes serve every step
    const bool padded = n < B && twin->graph_fits((n + 63) / 64 * 64);
    int n_eval = padded ? (n + 63) / 64 * 64 : n;
    if (n_eval > B) n_eval = B;
    last_refined = n;
    return refine_listed(r, R, B, n_eval, e_loc, stats, grad, logpsi, sign, skip_nl, padded ? d_flag.p : nullptr);
  }
  // step "probe": measure the float32 error per unit of score on a strided sample, re-derive the threshold
  // (refine_policy.h: refine_calibrate), and apply it to THIS call as well (a caller that evaluates once gets the calibrated
  // result)
  int refine_probed(const real* r, const real* R, int B, int n, real* e_loc, real* stats, real* grad, real* logpsi, int32_t* sign, bool skip_nl) {
    std::vector<int32_t> flagged((size_t)n);
    std::vector<double> score((size_t)B);
    std::vector<float> e32((size_t)B);
    if (n) HIP_TRY(hipMemcpyAsync(flagged.data(), d_flag + 1, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(score.data(), d_score, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(e32.data(), e_loc, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<char> done((size_t)B, 0);        // 1: evaluated in float64 by the first pass of this call (flagged or sample)
    for (int32_t b : flagged) if (b >= 0 && b < B) done[b] = 1;
    // calibration sample: a strided subset of the WHOLE batch (flagged or not: every walker is an (error, score) pair; a
    // system whose walkers all sit above the current threshold must still be able to move it)
    const int ns = B < refine_sample ? B : refine_sample;
    std::vector<int32_t> sample, list(flagged);
    std::vector<int> sample_pos;                 // position of each sample walker in `list`
    {
      std::vector<int> pos_of((size_t)B, -1);
      for (size_t k = 0; k < flagged.size(); ++k) if (flagged[k] >= 0 && flagged[k] < B) pos_of[flagged[k]] = (int)k;
      for (int j = 0; j < ns; ++j) {
        const int b = (int)((long)j * B / ns);
        if (pos_of[b] < 0) { pos_of[b] = (int)list.size(); list.push_back(b); done[b] = 1; }
        sample.push_back(b);
        sample_pos.push_back(pos_of[b]);
      }
    }
    // ONE float64 pass over flagged + sample; between its evaluation and its write-back the threshold is re-derived from
    // the sample, and only walkers above the NEW threshold are written back: what a walker's result is depends on its
    // score and the threshold alone -- never on having served as a calibration sample or on the threshold before the probe
    int rc = upload_list(list);
    if (rc) return rc;
    rc = refine_listed(r, R, B, (int)list.size(), e_loc, stats, grad, logpsi, sign, skip_nl, nullptr, [&](const std::vector<double>& e64) {
      std::vector<dqmc::RefineSample> cs;
      for (size_t k = 0; k < sample.size(); ++k) {
        const int32_t b = sample[k];
        const double e64v = e64[(size_t)sample_pos[k]];
        cs.push_back({std::fabs(e64v - (double)e32[b]) / std::fmax(1.0, std::fabs(e64v)), score[b]});
      }
      dqmc::refine_calibrate(cs, score.data(), B, refine_target, refine_miss, probe_c, refine_thresh);
    });
    if (rc) return rc;
    calls_since_probe = 0;
    long n_above = 0;
    for (int b = 0; b < B; ++b) if (!(score[b] <= refine_thresh)) ++n_above;
    std::vector<int32_t> more;
    if (refine == 1 && direct.decide(n_above, B)) {
      // most of the batch is beyond float32: the next calls go to float64 directly, and so does the rest of this one
      // (the few walkers below the threshold of such a system are not reliably predicted either)
      ++refine_counters[1];
      for (int b = 0; b < B; ++b) if (!done[b] || score[b] <= refine_thresh) more.push_back(b);     // not yet written back
      last_refined = B - (int)more.size();
    } else {
      for (int b = 0; b < B; ++b) {
        if (score[b] <= refine_thresh) continue;
        if (done[b]) ++last_refined; else more.push_back(b);
      }
    }
    if (more.empty()) return DQMC_OK;
    rc = upload_list(more);
    if (!rc) rc = refine_listed(r, R, B, (int)more.size(), e_loc, stats, grad, logpsi, sign, skip_nl);
    if (!rc) last_refined += (int)more.size();
    return rc;
  }

  // Effective core potentials: host tables (ecp/gaussian_type_ecp.py:32-93 layout) -> device.
  //   loc[n_nuc][3][2][n_t_loc]  r^-1 / r^0 / r^1 terms: [.,term,0,.] exponents, [.,term,1,.] coefficients
  //   nl [n_nuc][n_l][2][n_t_nl] channels l = 0..n_l-1; nuclei whose block is all zero have no non-local part
