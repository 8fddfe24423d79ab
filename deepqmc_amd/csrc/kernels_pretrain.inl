// kernels_pretrain.inl -- SCF-orbital pretraining (dqmc_pretrain_target, dqmc_orbitals, dqmc_orbitals_vjp,
// dqmc_pretrain_loss_grad).  Included by kernel_linear.hip after kernels_grad.inl.
//
// The target is a table-driven Cartesian GTO evaluation (reference pretrain/gto.py, pretrain/pretraining_target.py): per
// walker the atomic orbitals of every electron go to LDS, then every target entry contracts one LDS row with one column of
// mo_coeffs.  The tables (shells, primitives, mo_coeffs, confs) are the same for every walker and every thread of a wave reads
// them at addresses that differ by the column only, so they stay in the caches; the kernel is a few hundred flops per entry.
// The loss kernel turns orbitals and target into the per-walker loss and the cotangent of the ORBITALS buffer, which the
// Orbs mode of the reverse pass (engine_reverse.inl) carries on.  All arithmetic in `real`, the loss sums in double.

namespace dqmc {

// (2 l - 1)!! for l <= 3, (-1)!! = 1
__device__ __forceinline__ int pt_dfact(int l) { return l < 2 ? 1 : (l == 2 ? 3 : 15); }

__device__ __forceinline__ float pt_exp(float x) { return expf(x); }
__device__ __forceinline__ double pt_exp(double x) { return exp(x); }
__device__ __forceinline__ float pt_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double pt_abs(double x) { return fabs(x); }
__device__ __forceinline__ float pt_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double pt_sqrt(double x) { return sqrt(x); }

template <typename real>
__device__ __forceinline__ real pt_pow(real x, int n) {
  real p = 1;
  for (int k = 0; k < n; ++k) p *= x;
  return p;
}

// target[b][c][i][mu] = sum_ao phi_ao(r_i) mo[ao][confs[c][mu]] * fac[c][0] * (mu == 0 ? fac[c][1] : 1)
// shells: int32 [n_shell][PT_SHELL_INTS] = (atom, l, first primitive, primitives, first AO); prims: real [.][2] = (coeff x rnorm, zeta).
// One workgroup per walker (walker-stride loop); the electrons of a walker are taken e_tile at a time so that their AOs fit
// aos[PT_AO_CAP] (e_tile * n_ao <= PT_AO_CAP, checked by the host).
template <typename real>
__global__ void __launch_bounds__(256) k_pretrain_target(const real* __restrict__ r, const real* __restrict__ R,
                                                         const int32_t* __restrict__ shells, const real* __restrict__ prims,
                                                         const real* __restrict__ mo, const int32_t* __restrict__ confs,
                                                         const real* __restrict__ fac, real* __restrict__ target, int B, int N,
                                                         int n_shell, int n_ao, int n_mo, int n_conf, int e_tile) {
  __shared__ real aos[PT_AO_CAP];
  const int tid = threadIdx.x;
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    for (int i0 = 0; i0 < N; i0 += e_tile) {
      const int ne = N - i0 < e_tile ? N - i0 : e_tile;
      for (int t = tid; t < ne * n_shell; t += 256) {
        const int il = t / n_shell, s = t - il * n_shell;
        const int32_t* sh = shells + s * PT_SHELL_INTS;
        const int l = sh[1];
        const real x = r[(b * N + i0 + il) * 3 + 0] - R[sh[0] * 3 + 0];
        const real y = r[(b * N + i0 + il) * 3 + 1] - R[sh[0] * 3 + 1];
        const real z = r[(b * N + i0 + il) * 3 + 2] - R[sh[0] * 3 + 2];
        const real r2 = x * x + y * y + z * z;
        real radial = 0;
        for (int p = sh[2]; p < sh[2] + sh[3]; ++p) radial += prims[2 * p] * pt_exp(-pt_abs(prims[2 * p + 1] * r2));
        real* out = aos + il * n_ao + sh[4];
        for (int lx = l; lx >= 0; --lx)
          for (int ly = l - lx; ly >= 0; --ly) {
            const int lz = l - lx - ly;
            const real anorm = (real)1 / pt_sqrt((real)(pt_dfact(lx) * pt_dfact(ly) * pt_dfact(lz)));
            *out++ = anorm * (pt_pow(x, lx) * pt_pow(y, ly) * pt_pow(z, lz)) * radial;
          }
      }
      __syncthreads();
      for (int t = tid; t < n_conf * ne * N; t += 256) {
        const int mu = t % N, q = t / N;
        const int il = q % ne, c = q / ne;
        const int col = confs[c * N + mu];
        const real* a = aos + il * n_ao;
        real acc = 0;
        for (int ao = 0; ao < n_ao; ++ao) acc += a[ao] * mo[(long)ao * n_mo + col];
        const real f = mu == 0 ? fac[2 * c] * fac[2 * c + 1] : fac[2 * c];
        target[((b * n_conf + c) * N + i0 + il) * N + mu] = acc * f;
      }
      __syncthreads();
    }
  }
}

// dense[b][k][i*N + mu] <-> buf[b][k][orb_w] (the ORBITALS destination buffer of the value pass or its adjoint; the padding
// columns of the adjoint stay as the caller zeroed them)
template <typename real>
__global__ void __launch_bounds__(256) k_orbitals_copy(const real* __restrict__ src, long src_ld, real* __restrict__ dst, long dst_ld,
                                                       int NN, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int e = (int)(idx % NN);
  const long row = idx / NN;
  dst[row * dst_ld + e] = src[row * src_ld + e];
}

// Per walker (one workgroup each): loss[b] = mean_{k, i < n_up, mu} (A - T)^2 + mean_{k, i >= n_up, mu} (A - T)^2 and
// dorb[b][k][i*N + mu] = 2 (A - T) / (n_total K n_rows N), T[k] = configuration k mod n_conf of `target`, its up-up and
// down-down blocks only (zeros elsewhere).  inv_up / inv_dn = 1 / (K n_rows N), 0 for a spin without electrons.
template <typename real>
__global__ void __launch_bounds__(256) k_pretrain_loss(const real* __restrict__ orb, int orb_w, const real* __restrict__ target,
                                                       real* __restrict__ dorb, double* __restrict__ loss, int N, int n_up, int K,
                                                       int n_conf, double inv_up, double inv_dn, double n_total) {
  __shared__ double red[2][256];
  const long b = blockIdx.x;
  const int tid = threadIdx.x, NN = N * N;
  double su = 0, sd = 0;
  for (int t = tid; t < K * NN; t += 256) {
    const int k = t / NN, e = t - k * NN;
    const int i = e / N, mu = e - i * N;
    const bool up = i < n_up;
    const double tg = up == (mu < n_up) ? (double)target[((b * n_conf + k % n_conf) * N + i) * N + mu] : 0.0;
    const double d = (double)orb[(b * K + k) * orb_w + e] - tg;
    if (up) su += d * d; else sd += d * d;
    dorb[(b * K + k) * orb_w + e] = (real)(2.0 * d * (up ? inv_up : inv_dn) / n_total);
  }
  red[0][tid] = su; red[1][tid] = sd;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) loss[b] = red[0][0] * inv_up + red[1][0] * inv_dn;
}

template <typename real>
void launch_pretrain_target(hipStream_t st, const real* r, const real* R, const int32_t* shells, const real* prims, const real* mo,
                            const int32_t* confs, const real* fac, real* target, int B, int N, int n_shell, int n_ao, int n_mo,
                            int n_conf) {
  const int cap = PT_AO_CAP / n_ao, e_tile = cap < N ? cap : N;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pretrain_target<real>), dim3(B < 65535 ? B : 65535), dim3(256), 0, st, r, R, shells, prims, mo,
                     confs, fac, target, B, N, n_shell, n_ao, n_mo, n_conf, e_tile);
}
template <typename real>
void launch_orbitals_copy(hipStream_t st, const real* src, long src_ld, real* dst, long dst_ld, int NN, long rows) {
  const long n = rows * NN;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_orbitals_copy<real>), dim3(grad_grid(n)), dim3(256), 0, st, src, src_ld, dst, dst_ld, NN, n);
}
template <typename real>
void launch_pretrain_loss(hipStream_t st, const real* orb, int orb_w, const real* target, real* dorb, double* loss, int B, int N,
                          int n_up, int K, int n_conf, double n_total) {
  const double inv_up = n_up > 0 ? 1.0 / ((double)K * n_up * N) : 0.0, inv_dn = N > n_up ? 1.0 / ((double)K * (N - n_up) * N) : 0.0;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pretrain_loss<real>), dim3(B), dim3(256), 0, st, orb, orb_w, target, dorb, loss, N, n_up, K,
                     n_conf, inv_up, inv_dn, n_total);
}

#define DQMC_PRETRAIN_INST(real)                                                                                                   \
  template void launch_pretrain_target<real>(hipStream_t, const real*, const real*, const int32_t*, const real*, const real*,    \
                                             const int32_t*, const real*, real*, int, int, int, int, int, int);                  \
  template void launch_orbitals_copy<real>(hipStream_t, const real*, long, real*, long, int, long);                              \
  template void launch_pretrain_loss<real>(hipStream_t, const real*, int, const real*, real*, double*, int, int, int, int, int,  \
                                           double);
DQMC_PRETRAIN_INST(float)
DQMC_PRETRAIN_INST(double)
#undef DQMC_PRETRAIN_INST

}  // namespace dqmc
