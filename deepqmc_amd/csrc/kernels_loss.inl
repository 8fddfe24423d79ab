// kernels_loss.inl -- the loss assembly of multi-state training between the value passes and the reverse pass
// (dqmc_psi_ratio, dqmc_clip_rows, dqmc_loss_cotangents).  Included by kernel_linear.hip after kernels_optim.inl.
//
// Everything is double and small (S^2 rows of B walkers): what matters is that the assembly is three launches that never wait
// for the host, where the same formulas in torch are a sort and a dozen launches per row.  One workgroup owns one row.  Sums
// run in a fixed order (every thread its strided share in ascending order, a wave butterfly, four wave sums); the only atomics are
// integer counts of the radix select, whose result does not depend on their order: identical calls are bit-identical.
//
// The median is exact: a radix select over order-preserving 64-bit keys, eight passes of eight bits over the row in global
// memory (any B, no LDS tile of the row), and for even B the mean of the two middle values as jnp.median.

namespace dqmc {

// monotone map double -> uint64 (negative numbers: all bits flipped, others: sign bit set) and back
__device__ inline uint64_t loss_key(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double loss_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &u, 8);
  return x;
}

// sum of v over the workgroup, the same value in every thread, in a fixed order: a butterfly over the wave (lanes i and i ^ m
// add the same two numbers, so all 64 agree bit for bit), then the four wave sums through LDS (red: >= 4 doubles)
__device__ inline double loss_block_sum(double v, double* red) {
  static_assert(LOSS_BLOCK == 256, "four waves of 64");
  const int tid = threadIdx.x;
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                       // (red may still be read by the previous call)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The value a row element enters the select with: x itself, or its distance from `center`.
__device__ inline double loss_row_value(const double* __restrict__ x, long b, bool dev, double center) {
  const double v = x[b];
  return dev ? fabs(v - center) : v;
}

// key of the element of 0-based rank k of the row (ascending), the same value in every thread
__device__ inline uint64_t loss_select(const double* __restrict__ x, long B, long k, bool dev, double center, int* hist, uint64_t* sh) {
  const int tid = threadIdx.x;
  uint64_t prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    __syncthreads();
    hist[tid] = 0;                      // (LOSS_BLOCK == 256 bins)
    __syncthreads();
    for (long b = tid; b < B; b += LOSS_BLOCK) {
      const uint64_t key = loss_key(loss_row_value(x, b, dev, center));
      if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((key >> shift) & 255u)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      long seen = 0;
      int bin = 0;
      for (; bin < 255; ++bin) {
        if (seen + hist[bin] > k) break;
        seen += hist[bin];
      }
      sh[0] = prefix | ((uint64_t)bin << shift);
      sh[1] = (uint64_t)(k - seen);
    }
    __syncthreads();
    prefix = sh[0];
    k = (long)sh[1];
  }
  return prefix;
}

// median of the row values (or of their distances from `center`): the mean of the elements of ranks (B-1)/2 and B/2
__device__ inline double loss_median(const double* __restrict__ x, long B, bool dev, double center, int* hist, uint64_t* sh,
                                     uint64_t* kmin) {
  const int tid = threadIdx.x;
  const uint64_t k1 = loss_select(x, B, (B - 1) / 2, dev, center, hist, sh);
  const double lo = loss_unkey(k1);
  if (B % 2) return lo;
  // rank B/2: the same value if enough elements are <= it, else the smallest key above it
  long le = 0;
  uint64_t above = ~0ull;
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    const uint64_t key = loss_key(loss_row_value(x, b, dev, center));
    if (key <= k1) ++le;
    else if (key < above) above = key;
  }
  __syncthreads();
  hist[tid] = (int)le;
  kmin[tid] = above;
  __syncthreads();
  for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
      hist[tid] += hist[tid + s];
      if (kmin[tid + s] < kmin[tid]) kmin[tid] = kmin[tid + s];
    }
    __syncthreads();
  }
  const double hi = (long)hist[0] > B / 2 ? lo : loss_unkey(kmin[0]);
  return 0.5 * (lo + hi);
}

// one workgroup per row: centre, scale, clipped values, mask, row_stats[row] = {centre, scale, mean_b(w x_clip), mask count}
__global__ void __launch_bounds__(LOSS_BLOCK) k_clip_rows(const double* __restrict__ x, const double* __restrict__ w, long B, int center_kind,
                                                          int scale_kind, double clip_width, double exclude_width,
                                                          double* __restrict__ x_clip, uint8_t* __restrict__ mask,
                                                          double* __restrict__ row_stats) {
  __shared__ double red[LOSS_BLOCK];
  __shared__ int hist[LOSS_BLOCK];
  __shared__ uint64_t kmin[LOSS_BLOCK];
  __shared__ uint64_t sh[2];
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  x += row * B;
  x_clip += row * B;
  mask += row * B;
  if (w) w += row * B;
  const double nan = __builtin_nan("");

  // a non-finite input poisons the row: the select below still terminates (it only counts integer keys)
  double s = 0.0, bad = 0.0;
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    const double v = x[b];
    s += v;
    if (!(fabs(v) <= 1.79769313486231570e308)) bad += 1.0;
  }
  bad = loss_block_sum(bad, red);
  double center, scale;
  if (center_kind == LOSS_CENTER_MEDIAN) {
    center = loss_median(x, B, false, 0.0, hist, sh, kmin);
  } else {
    center = loss_block_sum(s, red) / (double)B;
  }
  if (scale_kind == LOSS_SCALE_MEDIAN_ABS_DEV) {
    scale = loss_median(x, B, true, center, hist, sh, kmin);
  } else {
    double a = 0.0;
    for (long b = tid; b < B; b += LOSS_BLOCK) a += fabs(x[b] - center);
    scale = loss_block_sum(a, red) / (double)B;
  }
  if (bad > 0.0) { center = nan; scale = nan; }
  const double lo = center - clip_width * scale, hi = center + clip_width * scale;
  double wx = 0.0, cnt = 0.0;
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    const double v = x[b];
    double c = v < lo ? lo : v;
    c = c > hi ? hi : c;
    if (bad > 0.0) c = nan;
    const bool m = fabs(v - center) < exclude_width;
    x_clip[b] = c;
    mask[b] = m ? 1 : 0;
    wx += (w ? w[b] : 1.0) * c;
    cnt += m ? 1.0 : 0.0;
  }
  wx = loss_block_sum(wx, red);
  cnt = loss_block_sum(cnt, red);
  if (tid == 0) {
    row_stats[4 * row + 0] = center;
    row_stats[4 * row + 1] = scale;
    row_stats[4 * row + 2] = wx / (double)B;
    row_stats[4 * row + 3] = cnt;
  }
}

// workgroup (i, j): ratio[i][j][b] = sign_ij sign_jj exp((log_ij - mean_i) - (log_jj - mean_j)), mean_i over all S B samples of
// wave function i (every workgroup sums the two means it needs itself, in the same order, so all agree bit for bit)
__global__ void __launch_bounds__(LOSS_BLOCK) k_psi_ratio(const double* __restrict__ lg, const double* __restrict__ sg, int S, long B,
                                                          double* __restrict__ ratio) {
  __shared__ double red[LOSS_BLOCK];
  const int tid = threadIdx.x;
  const int i = blockIdx.x / S, j = blockIdx.x % S;
  const long SB = (long)S * B;
  double si = 0.0, sj = 0.0;
  for (long e = tid; e < SB; e += LOSS_BLOCK) { si += lg[(long)i * SB + e]; sj += lg[(long)j * SB + e]; }
  const double mean_i = loss_block_sum(si, red) / (double)SB;
  const double mean_j = loss_block_sum(sj, red) / (double)SB;
  const double* lij = lg + ((long)i * S + j) * B;
  const double* ljj = lg + ((long)j * S + j) * B;
  const double* sij = sg + ((long)i * S + j) * B;
  const double* sjj = sg + ((long)j * S + j) * B;
  double* out = ratio + ((long)i * S + j) * B;
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    const double a = lij[b] - mean_i, d = ljj[b] - mean_j;
    out[b] = sij[b] * sjj[b] * exp(a - d);
  }
}

// workgroup j: the cotangent row c[j][:] of state j (formulas: include/dqmc.h, dqmc_loss_cotangents)
__global__ void __launch_bounds__(LOSS_BLOCK) k_loss_cotangents(LossCotArgs a) {
  __shared__ double red[LOSS_BLOCK];
  const int tid = threadIdx.x;
  const int j = blockIdx.x, S = a.S;
  const long B = a.B;
  const double* w = a.w ? a.w + (long)j * B : nullptr;
  double n_e = 0.0;
  for (int s = 0; s < S; ++s) n_e += a.e_stats[4 * s + 3];
  const double mean_e = a.e_stats[4 * j + 2];
  // the spin row of this state, if it is one of `states`
  int q = -1;
  double n_sp = 0.0, mu = 0.0;
  if (a.spin_kind != LOSS_SPIN_NONE) {
    for (int t = 0; t < a.n_states; ++t) {
      if (a.states[t] == j) q = t;      // (states: by value, range-checked by the host)
      n_sp += a.spin_kind == LOSS_SPIN_RAISING ? a.spin_stats[4 * t + 3] : a.e_stats[4 * a.states[t] + 3];
    }
    if (q >= 0 && a.spin_kind == LOSS_SPIN_RAISING) mu = a.spin_stats[4 * q + 2];
    if (a.spin_kind == LOSS_SPIN_SQUARED) {          // (every thread of the workgroup takes part, q >= 0 or not)
      double sw = 0.0;
      if (q >= 0) for (long b = tid; b < B; b += LOSS_BLOCK) sw += a.spin[(long)q * B + b] * (w ? w[b] : 1.0);
      mu = loss_block_sum(sw, red) / (double)B;
    }
  }
  const int rank_j = a.r_clip ? a.rank[j] : 0;
  for (long b = tid; b < B; b += LOSS_BLOCK) {
    const double wb = w ? w[b] : 1.0;
    const double me = a.e_mask[(long)j * B + b] ? 1.0 : 0.0;
    double c = me * wb * (a.e_clip[(long)j * B + b] - mean_e) / n_e;
    if (a.r_clip) {
      for (int i = 0; i < S; ++i) {
        if (a.rank[i] >= rank_j) continue;
        const long ij = (long)i * S + j, ji = (long)j * S + i;
        const double x_ij = a.r_stats[4 * ij + 2], x_ji = a.r_stats[4 * ji + 2], cnt = a.r_stats[4 * ij + 3];
        const double m = a.r_mask[ij * B + b] ? 1.0 : 0.0;
        c += a.alpha * (2.0 * x_ji * a.scale[ij]) * m * (a.r_clip[ij * B + b] - x_ij) * wb / cnt;
      }
    }
    if (q >= 0) {
      const long qb = (long)q * B + b;
      if (a.spin_kind == LOSS_SPIN_SQUARED) {
        c += a.lambda * me * wb * (a.spin[qb] - mu) / n_sp;
      } else {
        const double m = a.spin_mask[qb] ? 1.0 : 0.0;
        c += a.lambda * m * mu * wb * 2.0 * (a.spin[qb] - mu) / n_sp;
        if (a.k) a.k[qb] = a.lambda * m * mu * wb / n_sp;
      }
    }
    a.c[(long)j * B + b] = c;
  }
}

void launch_psi_ratio(hipStream_t st, const double* lg, const double* sg, int S, long B, double* ratio) {
  hipLaunchKernelGGL(k_psi_ratio, dim3((unsigned)(S * S)), dim3(LOSS_BLOCK), 0, st, lg, sg, S, B, ratio);
}
void launch_clip_rows(hipStream_t st, const double* x, const double* w, int n_rows, long B, int center_kind, int scale_kind,
                      double clip_width, double exclude_width, double* x_clip, uint8_t* mask, double* row_stats) {
  hipLaunchKernelGGL(k_clip_rows, dim3((unsigned)n_rows), dim3(LOSS_BLOCK), 0, st, x, w, B, center_kind, scale_kind, clip_width,
                     exclude_width, x_clip, mask, row_stats);
}
void launch_loss_cotangents(hipStream_t st, const LossCotArgs& a) {
  hipLaunchKernelGGL(k_loss_cotangents, dim3((unsigned)a.S), dim3(LOSS_BLOCK), 0, st, a);
}

}  // namespace dqmc
