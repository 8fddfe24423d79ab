// kernels_optim.inl -- the device-resident optimiser step (dqmc_set_param_map, dqmc_weights_from_params, dqmc_grad_to_params,
// dqmc_adam_step, dqmc_apply_update).  Included by kernel_linear.hip after kernels_pretrain.inl.
//
// Everything here moves a few MB at most: what matters is that a step is a handful of launches that never wait for the
// host.  The packed weight buffers are re-written by ONE table-driven kernel (k_pack_words): the host packers record, per
// destination word, where it comes from (kernels.h: PackSrc), so they stay the single definition of the layouts.  No
// atomics anywhere: the norms and the transpose of the packing sum in a fixed order, identical calls are bit-identical.

namespace dqmc {

struct alignas(16) OptWord4 { uint32_t x[4]; };
struct alignas(16) OptDouble2 { double x[2]; };

// piece pl (0..2) of the three-bf16 split of a float: round to nearest even, exact residuals -- bit for bit the bf16_piece
// of the host packers (engine_fused_plan.inl, spec_registry.hip).  The residual must be a plain subtraction: contracted into
// the product that formed v it would see the unrounded w * scale.
__device__ inline uint32_t opt_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return ((u >> 16) | 0x40u) & 0xffffu;
  return ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16) & 0xffffu;
}
__device__ inline uint32_t opt_bf16_piece(float v, int pl) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  uint32_t h = opt_bf16_rne(v);
  for (int k = 0; k < pl; ++k) {
    const uint32_t u = h << 16;
    float up;
    memcpy(&up, &u, 4);
    v = v - up;
    h = opt_bf16_rne(v);
  }
  return h;
}
// (float)w * scale rounded to float before anything else looks at it
template <typename real>
__device__ inline float opt_scaled(const real* __restrict__ w, int32_t src, float scale) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (src < 0) return 0.0f;
  const float v = (float)w[src] * scale;
  return v;
}

template <typename real>
__global__ void __launch_bounds__(OPT_BLOCK) k_weights_from_params(const double* __restrict__ theta, const int32_t* __restrict__ src,
                                                                   real* __restrict__ w, double* __restrict__ w64, long n) {
  for (long j = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; j < n; j += (long)gridDim.x * OPT_BLOCK) {
    const int32_t s = src[j];
    if (s < 0) continue;
    const double v = theta[s];
    w[j] = (real)v;
    if (w64) w64[j] = v;
  }
}

// float contexts: four 32-bit words per thread and one 16-byte store; the tail (n not a multiple of 4) word by word
__global__ void __launch_bounds__(OPT_BLOCK) k_pack_words_f32(const PackSrc* __restrict__ tab, const float* __restrict__ w,
                                                              uint32_t* __restrict__ out, long n) {
  const long n4 = (n + 3) / 4;
  for (long q4 = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; q4 < n4; q4 += (long)gridDim.x * OPT_BLOCK) {
    OptWord4 o;
    for (int k = 0; k < 4; ++k) {
      const long q = 4 * q4 + k;
      uint32_t word = 0;
      if (q < n) {
        const PackSrc t = tab[q];
        if (t.plane < 0) {
          const float v = opt_scaled(w, t.src0, t.scale);
          memcpy(&word, &v, 4);
        } else {
          word = opt_bf16_piece(opt_scaled(w, t.src0, t.scale), t.plane) | opt_bf16_piece(opt_scaled(w, t.src1, t.scale), t.plane) << 16;
        }
      }
      o.x[k] = word;
    }
    if (4 * q4 + 4 <= n) {
      *reinterpret_cast<OptWord4*>(out + 4 * q4) = o;
    } else {
      for (int k = 0; 4 * q4 + k < n; ++k) out[4 * q4 + k] = o.x[k];
    }
  }
}
// float64 contexts hold plain words only (no bf16 planes): two doubles per thread
__global__ void __launch_bounds__(OPT_BLOCK) k_pack_words_f64(const PackSrc* __restrict__ tab, const double* __restrict__ w,
                                                              double* __restrict__ out, long n) {
  const long n2 = (n + 1) / 2;
  for (long q2 = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; q2 < n2; q2 += (long)gridDim.x * OPT_BLOCK) {
    OptDouble2 o;
    for (int k = 0; k < 2; ++k) {
      const long q = 2 * q2 + k;
      double v = 0.0;
      if (q < n) {
        const PackSrc t = tab[q];
        if (t.src0 >= 0) v = w[t.src0] * (double)t.scale;
      }
      o.x[k] = v;
    }
    if (2 * q2 + 2 <= n) {
      *reinterpret_cast<OptDouble2*>(out + 2 * q2) = o;
    } else {
      out[2 * q2] = o.x[0];
    }
  }
}

__global__ void __launch_bounds__(OPT_BLOCK) k_grad_to_params(const double* __restrict__ grad_w, const int32_t* __restrict__ row,
                                                              const int32_t* __restrict__ col, double* __restrict__ grad_theta,
                                                              long n_params) {
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < n_params; e += (long)gridDim.x * OPT_BLOCK) {
    double s = 0.0;
    for (int32_t k = row[e]; k < row[e + 1]; ++k) s += grad_w[col[k]];
    grad_theta[e] = s;
  }
}

// the three sums of squares of one workgroup -> part[k][block], by a tree over LDS (fixed order)
__device__ inline void opt_block_sums(double a, double b, double c, double* __restrict__ part) {
  __shared__ double red[3][OPT_BLOCK];
  const int tid = threadIdx.x;
  red[0][tid] = a; red[1][tid] = b; red[2][tid] = c;
  __syncthreads();
  for (int s = OPT_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) for (int k = 0; k < 3; ++k) part[(long)k * OPT_MAX_BLOCKS + blockIdx.x] = red[k][0];
}

__global__ void __launch_bounds__(OPT_BLOCK) k_adam(double* __restrict__ theta, double* __restrict__ mu, double* __restrict__ nu,
                                                    const double* __restrict__ g, long n, double lr, double b1, double b2, double eps,
                                                    double c1, double c2, double* __restrict__ part) {
  double sp = 0, sg = 0, su = 0;
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * OPT_BLOCK) {
    const double ge = g[e], th = theta[e];
    const double m = b1 * mu[e] + (1 - b1) * ge;
    const double v = b2 * nu[e] + (1 - b2) * (ge * ge);
    const double upd = -lr * (m / c1) / (sqrt(v / c2) + eps);
    mu[e] = m; nu[e] = v; theta[e] = th + upd;
    sp += th * th; sg += ge * ge; su += upd * upd;
  }
  if (part) opt_block_sums(sp, sg, su, part);
}

__global__ void __launch_bounds__(OPT_BLOCK) k_apply_update(double* __restrict__ theta, const double* __restrict__ delta, double scale,
                                                            long n, double* __restrict__ part) {
  double sp = 0, sg = 0, su = 0;
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * OPT_BLOCK) {
    const double d = delta[e], th = theta[e], upd = scale * d;
    theta[e] = th + upd;
    sp += th * th; sg += d * d; su += upd * upd;
  }
  if (part) opt_block_sums(sp, sg, su, part);
}

// norms3[k] = sqrt(sum of part[k][0 .. nb)): every thread its strided share in ascending order, then the tree
__global__ void __launch_bounds__(OPT_BLOCK) k_norms_final(const double* __restrict__ part, int nb, double* __restrict__ norms3) {
  __shared__ double red[3][OPT_BLOCK];
  const int tid = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    double s = 0;
    for (int b = tid; b < nb; b += OPT_BLOCK) s += part[(long)k * OPT_MAX_BLOCKS + b];
    red[k][tid] = s;
  }
  __syncthreads();
  for (int s = OPT_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid < 3) norms3[tid] = sqrt(red[tid][0]);
}

inline int opt_grid(long n_items) {
  const long g = (n_items + OPT_BLOCK - 1) / OPT_BLOCK;
  return (int)(g < 1 ? 1 : (g > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : g));
}

template <typename real>
void launch_weights_from_params(hipStream_t st, const double* theta, const int32_t* src, real* w, double* w64, long n) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_weights_from_params<real>), dim3(opt_grid(n)), dim3(OPT_BLOCK), 0, st, theta, src, w, w64, n);
}
template <>
void launch_pack_words<float>(hipStream_t st, const PackSrc* tab, const float* w, float* out, long n) {
  hipLaunchKernelGGL(k_pack_words_f32, dim3(opt_grid((n + 3) / 4)), dim3(OPT_BLOCK), 0, st, tab, w, reinterpret_cast<uint32_t*>(out), n);
}
template <>
void launch_pack_words<double>(hipStream_t st, const PackSrc* tab, const double* w, double* out, long n) {
  hipLaunchKernelGGL(k_pack_words_f64, dim3(opt_grid((n + 1) / 2)), dim3(OPT_BLOCK), 0, st, tab, w, out, n);
}
void launch_grad_to_params(hipStream_t st, const double* grad_w, const int32_t* row, const int32_t* col, double* grad_theta,
                           long n_params) {
  hipLaunchKernelGGL(k_grad_to_params, dim3(opt_grid(n_params)), dim3(OPT_BLOCK), 0, st, grad_w, row, col, grad_theta, n_params);
}
void launch_adam(hipStream_t st, double* theta, double* mu, double* nu, const double* g, long n, double lr, double b1, double b2,
                 double eps, double c1, double c2, double* part, double* norms3) {
  const int nb = opt_grid(n);
  hipLaunchKernelGGL(k_adam, dim3(nb), dim3(OPT_BLOCK), 0, st, theta, mu, nu, g, n, lr, b1, b2, eps, c1, c2, norms3 ? part : nullptr);
  if (norms3) hipLaunchKernelGGL(k_norms_final, dim3(1), dim3(OPT_BLOCK), 0, st, (const double*)part, nb, norms3);
}
void launch_apply_update(hipStream_t st, double* theta, const double* delta, double scale, long n, double* part, double* norms3) {
  const int nb = opt_grid(n);
  hipLaunchKernelGGL(k_apply_update, dim3(nb), dim3(OPT_BLOCK), 0, st, theta, delta, scale, n, norms3 ? part : nullptr);
  if (norms3) hipLaunchKernelGGL(k_norms_final, dim3(1), dim3(OPT_BLOCK), 0, st, (const double*)part, nb, norms3);
}

template void launch_weights_from_params<float>(hipStream_t, const double*, const int32_t*, float*, double*, long);
template void launch_weights_from_params<double>(hipStream_t, const double*, const int32_t*, double*, double*, long);

}  // namespace dqmc
