// engine_observable.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the observables of the
// training loop that have kernels of their own (dqmc_oscillator_strength, dqmc_fd_displace, dqmc_fd_force; kernels_observable.inl).
//
// The context supplies its stream, its electron and nucleus counts and, for the oscillator strengths, a scratch of 2 S + 3 S^2
// doubles for the moments between the two launches (grow-only: allocated by the first call with a given S, kept afterwards).
// No call copies anything to the host or synchronises.

  DevBuf<double> os_mom;         // E mean [S], E std [S], cd std [S][S][3] of the last dqmc_oscillator_strength
  int os_S = 0;

  int oscillator_strength(const void* r, const double* ratio, const void* e_loc, int S, long B, double* os_mean, double* os_err,
                          double* cd_mean, double* cd_err) override {
    if (S < 1 || S > dqmc::LOSS_MAX_STATES) return fail(DQMC_E_ARG, "the number of states must lie in [1, " + std::to_string(dqmc::LOSS_MAX_STATES) + "]");
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    const int rc = os_mom.reserve((size_t)S * (2 + 3 * (size_t)S), st, "oscillator-strength moments");
    if (rc) return rc;
    os_S = S;
    dqmc::launch_oscillator_strength<real>(st, (const real*)r, ratio, (const real*)e_loc, S, B, N, os_mom, os_mean, os_err, cd_mean,
                                           cd_err);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  // dqmc_debug_read(-5): the moments of the last oscillator-strength call
  int read_os_moments(double* out, size_t n) {
    if (os_S == 0) return fail(DQMC_E_ARG, "no oscillator-strength call has run yet");
    const size_t cnt = (size_t)os_S * (2 + 3 * (size_t)os_S);
    if (n != cnt) return fail(DQMC_E_ARG, "size mismatch: expected " + std::to_string(cnt));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out, os_mom, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return DQMC_OK;
  }

  int fd_displace(const void* r, const void* R, long B, double h, void* r_out, void* R_out) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (r_out == r || R_out == R) return fail(DQMC_E_ARG, "the displaced copies must not alias their sources");
    dqmc::launch_fd_displace<real>(st, (const real*)r, (const real*)R, B, N, sys.n_nuc, h, (real*)r_out, (real*)R_out);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  int fd_force(const void* log_d, const void* log_0, const void* e_d, const void* e_0, long B, double h, double* F) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (!(h != 0.0)) return fail(DQMC_E_ARG, "the step size must not be zero");
    dqmc::launch_fd_force<real>(st, (const real*)log_d, (const real*)log_0, (const real*)e_d, (const real*)e_0, B, 3 * sys.n_nuc, h, F);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
