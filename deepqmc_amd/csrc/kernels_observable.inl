// kernels_observable.inl -- the observables of the training loop that have arithmetic of their own: oscillator strengths between
// electronic states (dqmc_oscillator_strength) and the finite-difference force (dqmc_fd_displace, dqmc_fd_force).  Included by
// kernels_ecp.hip, the way kernel_linear.hip includes the loss kernels.
//
// As the loss assembly: everything is double and small, what matters is that an observable is two launches that never wait for
// the host.  Sums run in a fixed order (every thread its strided share in ascending order, a wave butterfly, four wave sums: os_block_sum) and
// there are no atomics: identical calls are bit-identical.  The formulas stand in include/dqmc.h.

namespace dqmc {

// sum of v over the workgroup of LOSS_BLOCK threads, the same value in every thread, in a fixed order (loss_block_sum of
// kernels_loss.inl, which lives in another translation unit): a butterfly over the wave, then the four wave sums through LDS
__device__ inline double os_block_sum(double v, double* red) {
  static_assert(LOSS_BLOCK == 256, "four waves of 64");
  const int tid = threadIdx.x;
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                       // (red may still be read by the previous call)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the transition dipole sample of walker b of state j: d[c] = -sum_n r[j][b][n][c], the electrons added in ascending order
template <typename real>
__device__ inline void os_dipole(const real* __restrict__ r, long jb, int N, double d[3]) {
  const real* p = r + jb * N * 3;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int n = 0; n < N; ++n) { s0 += (double)p[3 * n]; s1 += (double)p[3 * n + 1]; s2 += (double)p[3 * n + 2]; }
  d[0] = -s0; d[1] = -s1; d[2] = -s2;
}

// workgroup (i, j): mean and population std over b of cd[i][j][b][c] = d[j][b][c] ratio[i][j][b] (two passes: the mean, then the
// squared deviations from it); workgroups (i, i) also those of e_loc[i].  mom: double[2 S + 3 S^2] = E mean [S], E std [S],
// cd std [S][S][3].
template <typename real>
__global__ void __launch_bounds__(LOSS_BLOCK) k_os_moments(const real* __restrict__ r, const double* __restrict__ ratio,
                                                           const real* __restrict__ e_loc, int S, long B, int N,
                                                           double* __restrict__ cd_mean, double* __restrict__ mom) {
  // no contraction: both passes must see the same ROUNDED product d ratio, or a fused d ratio - mean leaves the rounding error of
  // the product as a deviation (B = 1: a standard deviation of 1e-17 instead of 0, and 0 / 0 turns into a number downstream)
#pragma clang fp contract(off)
  __shared__ double red[LOSS_BLOCK];
  const int tid = threadIdx.x;
  const int i = blockIdx.x / S, j = blockIdx.x % S;
  const long ij = (long)i * S + j;
  const double* rho = ratio + ij * B;
  double s[3] = {0.0, 0.0, 0.0}, d[3];
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    os_dipole(r, (long)j * B + b, N, d);
    const double q = rho[b];
    for (int c = 0; c < 3; ++c) s[c] += d[c] * q;
  }
  double mean[3];
  for (int c = 0; c < 3; ++c) mean[c] = os_block_sum(s[c], red) / (double)B;
  double v[3] = {0.0, 0.0, 0.0};
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    os_dipole(r, (long)j * B + b, N, d);
    const double q = rho[b];
    for (int c = 0; c < 3; ++c) { const double x = d[c] * q - mean[c]; v[c] += x * x; }
  }
  for (int c = 0; c < 3; ++c) v[c] = sqrt(os_block_sum(v[c], red) / (double)B);
  if (tid == 0)
    for (int c = 0; c < 3; ++c) { cd_mean[3 * ij + c] = mean[c]; mom[2 * S + 3 * ij + c] = v[c]; }
  if (i != j) return;                     // (the same for the whole workgroup)
  const real* e = e_loc + (long)i * B;
  double se = 0.0;
  for (long b = tid; b < B; b += LOSS_BLOCK) se += (double)e[b];
  const double me = os_block_sum(se, red) / (double)B;
  double ve = 0.0;
  for (long b = tid; b < B; b += LOSS_BLOCK) { const double x = (double)e[b] - me; ve += x * x; }
  ve = sqrt(os_block_sum(ve, red) / (double)B);
  if (tid == 0) { mom[i] = me; mom[S + i] = ve; }
}

// one workgroup, a thread per ordered pair: error propagation from the moments to the oscillator strengths, every operation
// rounded on its own (no contraction into fused multiply-adds), in the order the header writes them
__global__ void __launch_bounds__(LOSS_BLOCK) k_os_finish(const double* __restrict__ cd_mean, const double* __restrict__ mom, int S, long B,
                                                          double* __restrict__ os_mean, double* __restrict__ os_err,
                                                          double* __restrict__ cd_err) {
#pragma clang fp contract(off)
  const double root_b = sqrt((double)B);
  const double* e_mean = mom;
  const double* e_std = mom + S;
  const double* cd_std = mom + 2 * S;
  for (int p = threadIdx.x; p < S * S; p += LOSS_BLOCK) {
    const int i = p / S, j = p % S;
    const long ij = (long)i * S + j, ji = (long)j * S + i;
    const double err_i = e_std[i] / root_b, err_j = e_std[j] / root_b;
    const double ex = e_mean[j] - e_mean[i];
    const double ex_err = sqrt(err_i * err_i + err_j * err_j);
    double ds = 0.0, ds_err2 = 0.0;
    for (int c = 0; c < 3; ++c) {
      const double err_ij = cd_std[3 * ij + c] / root_b, err_ji = cd_std[3 * ji + c] / root_b;
      const double rel_ij = err_ij / cd_mean[3 * ij + c], rel_ji = err_ji / cd_mean[3 * ji + c];
      const double ds_vec = cd_mean[3 * ij + c] * cd_mean[3 * ji + c];
      const double ds_err_vec = fabs(ds_vec) * sqrt(rel_ij * rel_ij + rel_ji * rel_ji);
      ds = ds + ds_vec;
      ds_err2 = ds_err2 + ds_err_vec * ds_err_vec;
      cd_err[3 * ij + c] = err_ij;
    }
    const double ds_err = sqrt(ds_err2);
    const double om = ((2.0 / 3.0) * ex) * ds;
    const double q_ex = ex_err / ex, q_ds = ds_err / ds;
    os_mean[ij] = om;
    os_err[ij] = ((2.0 / 3.0) * fabs(om)) * sqrt(q_ex * q_ex + q_ds * q_ds);
  }
}

// thread (b, e): the weights w[n] = exp(-|R_n - r_be|) / sum_n' exp(-|R_n' - r_be|) in double, and the electron's row of all
// D = 3 n_nuc displaced copies, r_out[d = 3 n0 + j0][b][e][j] = r[b][e][j] + [j == j0] h w[n0].  The first 3 D n_nuc threads
// also write the displaced geometries R_out[d][n][j] = R[n][j] - [n == n0][j == j0] h.
template <typename real>
__global__ void __launch_bounds__(256) k_fd_displace(const real* __restrict__ r, const real* __restrict__ R, long B, int N, int n_nuc,
                                                     double h, real* __restrict__ r_out, real* __restrict__ R_out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int D = 3 * n_nuc;
  if (idx < (long)D * D) {
    const int d = (int)(idx / D), nj = (int)(idx % D);
    const double x = (double)R[nj];
    R_out[idx] = (real)(nj == d ? x - h : x);
  }
  if (idx >= B * N) return;
  const double x[3] = {(double)r[3 * idx], (double)r[3 * idx + 1], (double)r[3 * idx + 2]};
  double sum = 0.0;
  for (int n = 0; n < n_nuc; ++n) {
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c) { const double t = (double)R[3 * n + c] - x[c]; d2 += t * t; }
    sum += exp(-sqrt(d2));
  }
  const long BN3 = B * N * 3;
  for (int n = 0; n < n_nuc; ++n) {
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c) { const double t = (double)R[3 * n + c] - x[c]; d2 += t * t; }
    const double w = exp(-sqrt(d2)) / sum;
    for (int j0 = 0; j0 < 3; ++j0) {
      real* o = r_out + (long)(3 * n + j0) * BN3 + 3 * idx;
      for (int c = 0; c < 3; ++c) o[c] = (real)(c == j0 ? x[c] + h * w : x[c]);
    }
  }
}

// F[b][d] = exp(2 (log_d[d][b] - log_0[b])) ((e_d[d][b] - e_0[b]) / h), double
template <typename real>
__global__ void __launch_bounds__(256) k_fd_force(const real* __restrict__ log_d, const real* __restrict__ log_0, const real* __restrict__ e_d,
                                                  const real* __restrict__ e_0, long B, int D, double h, double* __restrict__ F) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * D) return;
  const long b = idx / D;
  const int d = (int)(idx % D);
  const double w = exp(2.0 * ((double)log_d[(long)d * B + b] - (double)log_0[b]));
  F[idx] = w * (((double)e_d[(long)d * B + b] - (double)e_0[b]) / h);
}

template <typename real>
void launch_oscillator_strength(hipStream_t st, const real* r, const double* ratio, const real* e_loc, int S, long B, int N, double* mom,
                                double* os_mean, double* os_err, double* cd_mean, double* cd_err) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_os_moments<real>), dim3((unsigned)(S * S)), dim3(LOSS_BLOCK), 0, st, r, ratio, e_loc, S, B, N,
                     cd_mean, mom);
  hipLaunchKernelGGL(k_os_finish, dim3(1), dim3(LOSS_BLOCK), 0, st, (const double*)cd_mean, (const double*)mom, S, B, os_mean, os_err,
                     cd_err);
}

template <typename real>
void launch_fd_displace(hipStream_t st, const real* r, const real* R, long B, int N, int n_nuc, double h, real* r_out, real* R_out) {
  const long D = 3 * n_nuc, n = B * N > D * D ? B * N : D * D;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fd_displace<real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r, R, B, N, n_nuc, h,
                     r_out, R_out);
}

template <typename real>
void launch_fd_force(hipStream_t st, const real* log_d, const real* log_0, const real* e_d, const real* e_0, long B, int D, double h,
                     double* F) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fd_force<real>), dim3((unsigned)((B * D + 255) / 256)), dim3(256), 0, st, log_d, log_0, e_d, e_0,
                     B, D, h, F);
}

#define DQMC_OBSERVABLE_INST(real)                                                                                                  \
  template void launch_oscillator_strength<real>(hipStream_t, const real*, const double*, const real*, int, long, int, double*,    \
                                                 double*, double*, double*, double*);                                              \
  template void launch_fd_displace<real>(hipStream_t, const real*, const real*, long, int, int, double, real*, real*);             \
  template void launch_fd_force<real>(hipStream_t, const real*, const real*, const real*, const real*, long, int, double, double*);
DQMC_OBSERVABLE_INST(float)
DQMC_OBSERVABLE_INST(double)
#undef DQMC_OBSERVABLE_INST

}  // namespace dqmc
