// engine_loss.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the loss assembly of
// multi-state training (dqmc_psi_ratio, dqmc_clip_rows, dqmc_loss_cotangents; kernels_loss.inl).
//
// The context supplies its stream and nothing else: the kernels keep their scratch in LDS, so a call allocates nothing,
// copies nothing to the host and never synchronises.  All buffers are the caller's, double (masks: one byte per element).
// The public DQMC_CLIP_* / DQMC_SPIN_* values are handed to the kernels as they are: they must be the kernels' LOSS_* enums.

  static_assert(DQMC_CLIP_CENTER_MEAN == dqmc::LOSS_CENTER_MEAN && DQMC_CLIP_CENTER_MEDIAN == dqmc::LOSS_CENTER_MEDIAN, "centre kinds");
  static_assert(DQMC_CLIP_SCALE_MEAN_ABS_DEV == dqmc::LOSS_SCALE_MEAN_ABS_DEV &&
                DQMC_CLIP_SCALE_MEDIAN_ABS_DEV == dqmc::LOSS_SCALE_MEDIAN_ABS_DEV, "scale kinds");
  static_assert(DQMC_SPIN_NONE == dqmc::LOSS_SPIN_NONE && DQMC_SPIN_SQUARED == dqmc::LOSS_SPIN_SQUARED &&
                DQMC_SPIN_RAISING == dqmc::LOSS_SPIN_RAISING, "spin penalty kinds");

  int psi_ratio(const double* lg, const double* sg, int S, long B, double* ratio) override {
    if (S < 1 || S > dqmc::LOSS_MAX_STATES) return fail(DQMC_E_ARG, "the number of states must lie in [1, " + std::to_string(dqmc::LOSS_MAX_STATES) + "]");
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    dqmc::launch_psi_ratio(st, lg, sg, S, B, ratio);
    return DQMC_OK;
  }

  int clip_rows(const double* x, const double* w, int n_rows, long B, int center, int scale, double clip_width, double exclude_width,
                double* x_clip, uint8_t* mask, double* row_stats) override {
    if (n_rows < 1 || B < 1) return fail(DQMC_E_ARG, "n_rows and B must be positive");
    if (center != DQMC_CLIP_CENTER_MEAN && center != DQMC_CLIP_CENTER_MEDIAN) return fail(DQMC_E_ARG, "unknown centre");
    if (scale != DQMC_CLIP_SCALE_MEAN_ABS_DEV && scale != DQMC_CLIP_SCALE_MEDIAN_ABS_DEV) return fail(DQMC_E_ARG, "unknown scale");
    if (x == x_clip) return fail(DQMC_E_ARG, "x_clip must not alias x");
    dqmc::launch_clip_rows(st, x, w, n_rows, B, center, scale, clip_width, exclude_width, x_clip, mask, row_stats);
    return DQMC_OK;
  }

  int loss_cotangents(const dqmc_loss_terms* t, double* c, double* k) override {
    if (t->S < 1 || t->S > dqmc::LOSS_MAX_STATES) return fail(DQMC_E_ARG, "the number of states must lie in [1, " + std::to_string(dqmc::LOSS_MAX_STATES) + "]");
    if (t->B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (!t->e_clip || !t->e_mask || !t->e_stats) return fail(DQMC_E_ARG, "the clipped energies, their mask and row statistics are required");
    if (t->r_clip && (!t->r_mask || !t->r_stats || !t->scale || !t->rank)) return fail(DQMC_E_ARG, "the overlap term needs r_mask, r_stats, scale and rank");
    dqmc::LossCotArgs a{};
    a.S = t->S; a.B = t->B; a.w = t->w;
    a.e_clip = t->e_clip; a.e_mask = t->e_mask; a.e_stats = t->e_stats;
    a.alpha = t->alpha; a.r_clip = t->r_clip; a.r_mask = t->r_mask; a.r_stats = t->r_stats; a.scale = t->scale; a.rank = t->rank;
    a.spin_kind = t->spin_kind; a.lambda = t->lambda; a.spin = t->spin; a.spin_mask = t->spin_mask; a.spin_stats = t->spin_stats;
    a.n_states = 0;
    if (t->spin_kind != DQMC_SPIN_NONE) {
      if (t->spin_kind != DQMC_SPIN_SQUARED && t->spin_kind != DQMC_SPIN_RAISING) return fail(DQMC_E_ARG, "unknown spin penalty kind");
      if (!t->spin || !t->states_host || t->n_states < 1 || t->n_states > t->S) return fail(DQMC_E_ARG, "the spin term needs its rows and 1..S states");
      if (t->spin_kind == DQMC_SPIN_RAISING && (!t->spin_mask || !t->spin_stats)) return fail(DQMC_E_ARG, "the raising kind needs the mask and row statistics of its clipped rows");
      for (int q = 0; q < t->n_states; ++q) {
        if (t->states_host[q] < 0 || t->states_host[q] >= t->S) return fail(DQMC_E_ARG, "spin state " + std::to_string(t->states_host[q]) + " is out of range");
        for (int p = 0; p < q; ++p) if (t->states_host[p] == t->states_host[q]) return fail(DQMC_E_ARG, "spin states must be distinct");
        a.states[q] = t->states_host[q];
      }
      a.n_states = t->n_states;
    }
    a.c = c; a.k = t->spin_kind == DQMC_SPIN_RAISING ? k : nullptr;
    dqmc::launch_loss_cotangents(st, a);
    return DQMC_OK;
  }
