// kernels_coords.inl -- coordinate reverse pass (dqmc_log_psi_grad_coords) and the Hellmann-Feynman force estimators
// (dqmc_hf_force).  Included by kernel_linear.hip after kernels_grad.inl.
//
// Every op that reads the coordinates reads them through differences d = r_p - r_q (p an electron, q an electron or a
// nucleus).  The backward kernels below map the adjoints of such an op to a 3-vector dd = d log|psi| / d d per difference
// ("slot", double[B][n_slots][3]); the slots an op writes are its own, and `slot` points at the first of them.  k_coords_gather then sums, for every particle, the
// slots it enters with + (p) or - (q) in the fixed order of a host-built table: no atomics, bit-identical repeats.

namespace dqmc {

// dd of the pair features [rho, d] (log_rescale: [log1p rho, d log1p(rho) / rho]), rho = sqrt(eps + d.d), given their adjoint g
__device__ __forceinline__ void pair_feature_bwd(const double d[3], double eps, bool log_rescale, const double g[4], double dd[3]) {
  const double rho = sqrt(eps + d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (!log_rescale) {
    for (int a = 0; a < 3; ++a) dd[a] = g[0] * d[a] / rho + g[1 + a];
    return;
  }
  const double s = log1p(rho) / rho, s1 = (1.0 / (1.0 + rho) - s) / rho;       // s(rho), s'(rho)
  const double gd = g[1] * d[0] + g[2] * d[1] + g[3] * d[2];
  const double c = (g[0] / (1.0 + rho) + gd * s1) / rho;
  for (int a = 0; a < 3; ++a) dd[a] = c * d[a] + g[1 + a] * s;
}

// FEAT_EN: slot (i, a) of walker b, d = r_i - R_a, from the adjoint row dx[b][i][4a .. 4a+3]
template <typename real>
__global__ void __launch_bounds__(256) k_feat_en_coords(const real* __restrict__ r, const real* __restrict__ R, const real* __restrict__ dx,
                                                        int width, int N, int n_nuc, double eps, int log_rescale,
                                                        double* __restrict__ slot, int n_slots, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int a = (int)(idx % n_nuc);
  const long q = idx / n_nuc;
  const int i = (int)(q % N);
  const long b = q / N;
  double d[3], g[4], dd[3];
  for (int c = 0; c < 3; ++c) d[c] = (double)r[(b * N + i) * 3 + c] - (double)R[a * 3 + c];
  for (int c = 0; c < 4; ++c) g[c] = (double)dx[(b * N + i) * width + 4 * a + c];
  pair_feature_bwd(d, eps, log_rescale != 0, g, dd);
  double* o = slot + (b * n_slots + (long)i * n_nuc + a) * 3;
  for (int c = 0; c < 3; ++c) o[c] = dd[c];
}

// FEAT_EE: slot `row` of walker b, d = r_recv - r_send (a negative sender s: nucleus -1 - s), from the adjoint de[b][row][0..3]
template <typename real>
__global__ void __launch_bounds__(256) k_feat_ee_coords(const real* __restrict__ r, const real* __restrict__ R,
                                                        const int32_t* __restrict__ pairs, const real* __restrict__ de, int n_rows,
                                                        int N, double eps, int log_rescale, double* __restrict__ slot, int n_slots,
                                                        long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % n_rows);
  const long b = idx / n_rows;
  const int rc = pairs[2 * k], sd = pairs[2 * k + 1];
  double d[3], g[4], dd[3];
  for (int c = 0; c < 3; ++c)
    d[c] = (double)r[(b * N + rc) * 3 + c] - (sd >= 0 ? (double)r[(b * N + sd) * 3 + c] : (double)R[(-1 - sd) * 3 + c]);
  for (int c = 0; c < 4; ++c) g[c] = (double)de[(b * n_rows + k) * 4 + c];
  pair_feature_bwd(d, eps, log_rescale != 0, g, dd);
  double* o = slot + (b * n_slots + k) * 3;
  for (int c = 0; c < 3; ++c) o[c] = dd[c];
}

// ORBITALS: slot (i, a) of walker b, d = r_i - R_a: the envelopes env_i[o] = sum_e pi[o][a n_env + e] exp(-|zeta| rho_ia) of
// electron i's spin, weighted by the adjoint of A_k[i][mu] = env_i[o] bf[i][o] (o = k N + mu)
template <typename real>
__global__ void __launch_bounds__(256) k_orbitals_coords(const real* __restrict__ r, const real* __restrict__ R, const real* __restrict__ bf,
                                                         int bf_w, const real* __restrict__ dorb, int orb_w, const real* __restrict__ pi_up,
                                                         const real* __restrict__ pi_dn, const real* __restrict__ ze_up,
                                                         const real* __restrict__ ze_dn, int N, int n_up, int n_env, int n_nuc, int K,
                                                         double eps, double* __restrict__ slot, int n_slots, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int a = (int)(idx % n_nuc);
  const long q = idx / n_nuc;
  const int i = (int)(q % N);
  const long b = q / N;
  const int L = n_nuc * n_env, KN = K * N;
  const real* pi = i < n_up ? pi_up : pi_dn;
  const real* ze = i < n_up ? ze_up : ze_dn;
  double d[3], d2 = eps;
  for (int c = 0; c < 3; ++c) { d[c] = (double)r[(b * N + i) * 3 + c] - (double)R[a * 3 + c]; d2 += d[c] * d[c]; }
  const double rho = sqrt(d2);
  double s = 0;     // d log|psi| / d rho_ia
  for (int o = 0; o < KN; ++o) {
    const int k = o / N, mu = o - k * N;
    const double t = (double)dorb[(b * K + k) * orb_w + i * N + mu] * (double)bf[(b * N + i) * bf_w + o];
    for (int e = 0; e < n_env; ++e) {
      const double az = fabs((double)ze[(long)o * L + a * n_env + e]);
      s -= t * (double)pi[(long)o * L + a * n_env + e] * az * exp(-az * rho);
    }
  }
  double* out = slot + (b * n_slots + (long)i * n_nuc + a) * 3;
  for (int c = 0; c < 3; ++c) out[c] = s * d[c] / rho;
}

// FINAL: slot p of walker b for the electron pair p = (i, j), i < j, row-major: d = r_i - r_j, the derivative of the pair
// cusp term (kernels_head.hip) along d
template <typename real>
__global__ void __launch_bounds__(256) k_cusp_coords(const real* __restrict__ r, const real* __restrict__ alphas, int cusp_kind,
                                                     double same_scale, double anti_scale, double eps, int N, int n_up,
                                                     double* __restrict__ slot, int n_slots, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int n_pairs = N * (N - 1) / 2;
  const int p = (int)(idx % n_pairs);
  const long b = idx / n_pairs;
  int i = 0, p0 = 0;
  while (p - p0 >= N - 1 - i) { p0 += N - 1 - i; ++i; }
  const int j = i + 1 + (p - p0);
  double d[3], d2 = eps;
  for (int c = 0; c < 3; ++c) { d[c] = (double)r[(b * N + i) * 3 + c] - (double)r[(b * N + j) * 3 + c]; d2 += d[c] * d[c]; }
  const double rho = sqrt(d2);
  const bool same = (i < n_up) == (j < n_up);
  const double sc = same ? same_scale : anti_scale, al = (double)alphas[same ? 0 : 1];
  const double g1 = cusp_kind == 1 ? sc / ((1 + al * rho) * (1 + al * rho)) : sc * al * al / ((al + rho) * (al + rho));
  double* o = slot + (b * n_slots + p) * 3;
  for (int c = 0; c < 3; ++c) o[c] = g1 * d[c] / rho;
}

// grad[b][particle] = sum over tab[particle][S] = (slot, +-1) of sign * dd[b][slot]; particles 0 .. N-1 are the electrons
// (-> grad_r), N .. N + n_nuc - 1 the nuclei (-> grad_R).  Walkers with sign 0 or a non-finite log|psi| get zero rows.
template <typename real>
__global__ void __launch_bounds__(256) k_coords_gather(const double* __restrict__ slot, int n_slots, const int32_t* __restrict__ tab, int S,
                                                       const real* __restrict__ lp, const int32_t* __restrict__ sg, int N, int n_nuc,
                                                       real* __restrict__ grad_r, real* __restrict__ grad_R, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int P = N + n_nuc;
  const int p = (int)(idx % P);
  const long b = idx / P;
  real* out = p < N ? (grad_r ? grad_r + (b * N + p) * 3 : nullptr) : (grad_R ? grad_R + (b * n_nuc + p - N) * 3 : nullptr);
  if (!out) return;
  const double l = (double)lp[b];
  double s[3] = {0, 0, 0};
  if (sg[b] != 0 && l - l == 0) {
    for (int e = 0; e < S; ++e) {
      const int k = tab[(p * S + e) * 2], w = tab[(p * S + e) * 2 + 1];
      if (k < 0) break;
      const double* v = slot + ((long)b * n_slots + k) * 3;
      for (int c = 0; c < 3; ++c) s[c] += w * v[c];
    }
  }
  for (int c = 0; c < 3; ++c) out[c] = (real)s[c];
}

// ---- Hellmann-Feynman force estimators (dqmc_hf_force; estimator codes of include/dqmc.h) ----
// One thread per (walker, nucleus I); double throughout.  d = r_i - R_I, rho = |d|, u = d / rho.
template <typename real>
__global__ void __launch_bounds__(256) k_hf_force(int est, const real* __restrict__ r, const real* __restrict__ R,
                                                  const double* __restrict__ Z, const real* __restrict__ gr, const real* __restrict__ gR,
                                                  const real* __restrict__ e_loc, double energy, int N, int n_nuc,
                                                  double* __restrict__ force, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int I = (int)(idx % n_nuc);
  const long b = idx / n_nuc;
  double f[3] = {0, 0, 0};
  for (int J = 0; J < n_nuc; ++J) {           // nuclear repulsion, -grad_R_I of sum_{I<J} Z_I Z_J / |R_I - R_J|
    if (J == I) continue;
    double d[3], d2 = 0;
    for (int c = 0; c < 3; ++c) { d[c] = (double)R[I * 3 + c] - (double)R[J * 3 + c]; d2 += d[c] * d[c]; }
    const double w = Z[I] * Z[J] / (d2 * sqrt(d2));
    for (int c = 0; c < 3; ++c) f[c] += w * d[c];
  }
  if (est != DQMC_FORCE_NUCLEAR) {
    const bool zvq = est == DQMC_FORCE_AC_ZVQ || est == DQMC_FORCE_AC_ZVZBQ || est == DQMC_FORCE_AC_ZVQZB;
    double fe[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    for (int i = 0; i < N; ++i) {
      double d[3], d2 = 0;
      for (int c = 0; c < 3; ++c) { d[c] = (double)r[(b * N + i) * 3 + c] - (double)R[I * 3 + c]; d2 += d[c] * d[c]; }
      const double rho = sqrt(d2);
      double u[3];
      for (int c = 0; c < 3; ++c) u[c] = d[c] / rho;
      if (zvq) {      // grad_r log psi . grad_r Q_I: (g_i - (u . g_i) u) / rho
        double g[3];
        for (int c = 0; c < 3; ++c) g[c] = (double)gr[(b * N + i) * 3 + c];
        const double ug = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
        for (int c = 0; c < 3; ++c) fe[c] += (g[c] - ug * u[c]) / rho;
        for (int c = 0; c < 3; ++c) q[c] += u[c];
      } else {        // bare: -grad_R_I of the electron-nucleus attraction
        for (int c = 0; c < 3; ++c) fe[c] += d[c] / (d2 * rho);
      }
    }
    for (int c = 0; c < 3; ++c) f[c] += Z[I] * fe[c];
    const double de = est == DQMC_FORCE_AC_ZVZBQ || est == DQMC_FORCE_AC_ZB || est == DQMC_FORCE_AC_ZVQZB
                          ? -2.0 * ((double)e_loc[b] - energy) : 0.0;
    if (est == DQMC_FORCE_AC_ZVZBQ)
      for (int c = 0; c < 3; ++c) f[c] += de * Z[I] * q[c];
    else if (est == DQMC_FORCE_AC_ZB || est == DQMC_FORCE_AC_ZVQZB)
      for (int c = 0; c < 3; ++c) f[c] += de * (double)gR[(b * n_nuc + I) * 3 + c];
  }
  for (int c = 0; c < 3; ++c) force[idx * 3 + c] = f[c];
}

// ---- launchers ----

template <typename real>
void launch_feat_en_coords(hipStream_t st, const real* r, const real* R, const real* dx, int width, int B, int N, int n_nuc, double eps,
                           int log_rescale, double* slot, int n_slots) {
  const long n = (long)B * N * n_nuc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_en_coords<real>), dim3(grad_grid(n)), dim3(256), 0, st, r, R, dx, width, N, n_nuc, eps,
                     log_rescale, slot, n_slots, n);
}
template <typename real>
void launch_feat_ee_coords(hipStream_t st, const real* r, const real* R, const int32_t* pairs, const real* de, int n_rows, int B, int N,
                           double eps, int log_rescale, double* slot, int n_slots) {
  const long n = (long)B * n_rows;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_feat_ee_coords<real>), dim3(grad_grid(n)), dim3(256), 0, st, r, R, pairs, de, n_rows, N, eps,
                     log_rescale, slot, n_slots, n);
}
template <typename real>
void launch_orbitals_coords(hipStream_t st, const real* r, const real* R, const real* bf, int bf_w, const real* dorb, int orb_w,
                            const real* pi_up, const real* pi_dn, const real* ze_up, const real* ze_dn, int B, int N, int n_up, int n_env,
                            int n_nuc, int K, double eps, double* slot, int n_slots) {
  const long n = (long)B * N * n_nuc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_orbitals_coords<real>), dim3(grad_grid(n)), dim3(256), 0, st, r, R, bf, bf_w, dorb, orb_w, pi_up,
                     pi_dn, ze_up, ze_dn, N, n_up, n_env, n_nuc, K, eps, slot, n_slots, n);
}
template <typename real>
void launch_cusp_coords(hipStream_t st, const real* r, const real* alphas, int cusp_kind, double same_scale, double anti_scale,
                        double eps, int B, int N, int n_up, double* slot, int n_slots) {
  const long n = (long)B * (N * (N - 1) / 2);
  if (n > 0)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cusp_coords<real>), dim3(grad_grid(n)), dim3(256), 0, st, r, alphas, cusp_kind, same_scale,
                       anti_scale, eps, N, n_up, slot, n_slots, n);
}
template <typename real>
void launch_coords_gather(hipStream_t st, const double* slot, int n_slots, const int32_t* tab, int S, const real* lp, const int32_t* sg,
                          int B, int N, int n_nuc, real* grad_r, real* grad_R) {
  const long n = (long)B * (N + n_nuc);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_coords_gather<real>), dim3(grad_grid(n)), dim3(256), 0, st, slot, n_slots, tab, S, lp, sg, N,
                     n_nuc, grad_r, grad_R, n);
}
template <typename real>
void launch_hf_force(hipStream_t st, int est, const real* r, const real* R, const double* Z, const real* gr, const real* gR,
                     const real* e_loc, double energy, int B, int N, int n_nuc, double* force) {
  const long n = (long)B * n_nuc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hf_force<real>), dim3(grad_grid(n)), dim3(256), 0, st, est, r, R, Z, gr, gR, e_loc, energy, N,
                     n_nuc, force, n);
}

#define DQMC_COORDS_INST(real)                                                                                                      \
  template void launch_feat_en_coords<real>(hipStream_t, const real*, const real*, const real*, int, int, int, int, double, int,   \
                                            double*, int);                                                                        \
  template void launch_feat_ee_coords<real>(hipStream_t, const real*, const real*, const int32_t*, const real*, int, int, int,    \
                                            double, int, double*, int);                                                           \
  template void launch_orbitals_coords<real>(hipStream_t, const real*, const real*, const real*, int, const real*, int,          \
                                             const real*, const real*, const real*, const real*, int, int, int, int, int, int,   \
                                             double, double*, int);                                                               \
  template void launch_cusp_coords<real>(hipStream_t, const real*, const real*, int, double, double, double, int, int, int,      \
                                         double*, int);                                                                           \
  template void launch_coords_gather<real>(hipStream_t, const double*, int, const int32_t*, int, const real*, const int32_t*,    \
                                           int, int, int, real*, real*);                                                          \
  template void launch_hf_force<real>(hipStream_t, int, const real*, const real*, const double*, const real*, const real*,        \
                                      const real*, double, int, int, int, double*);
DQMC_COORDS_INST(float)
DQMC_COORDS_INST(double)
#undef DQMC_COORDS_INST

}  // namespace dqmc
