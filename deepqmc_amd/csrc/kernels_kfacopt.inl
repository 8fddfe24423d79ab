// kernels_kfacopt.inl -- the KFAC preconditioner on the flat device vectors (dqmc_set_kfac_map, dqmc_kfac_direction,
// dqmc_kfac_apply).  Included by kernel_linear.hip after kernels_optim.inl (whose block reductions it reuses).
//
// One direction is a fixed launch sequence on the context's stream, float64 throughout:
//   k_kf_count     n_v from sign / log|psi| (the validity rule of k_kfac_weights)
//   k_kf_assemble  per element of every module's A_hat / G_hat: the per-op factors gathered through the inverse row / column
//                  maps in op order, normalised, mixed into the state (EMA)
//   k_kf_diag      F_ii of the diagonal elements from `rest` (four walker slices per element, combined in a fixed order), the
//                  EMA and delta_i = g_i / (F_ii + damping)
//   k_kf_pi        tr A_hat, tr G_hat -> pi per module
//   k_kf_load      M = factor + its damping on the diagonal, for every matrix
//   k_kf_panel / k_kf_trail, once per panel index: blocked right-looking Cholesky M = L L^T of ALL matrices in lockstep.  The
//                  matrices are sorted by dimension, descending, so the ones that still have a panel k form a prefix of the list
//                  and a small matrix is finished after its own few panels; launch k covers that prefix only.  The KF_NB x KF_NB
//                  diagonal block is factored in LDS (every workgroup of the matrix does it for itself, the first one stores
//                  it), the rows below are solved against it one per thread, and the trailing matrix is updated from global
//                  memory by v_mfma_f64_16x16x4_f64, one 16 x 16 tile per wave.
//   k_kf_solve x4  [W; b] <- A_d^-1 [W; b] G_d^-1 as four blocked triangular solves with many right-hand sides, in place in
//                  delta (which starts as a copy of the gradient): KF_RB right-hand sides per workgroup, the part left (right)
//                  of a KF_NB block as dot products from global memory, the block itself in LDS.
//   k_kf_dot       <delta, g>, block partials and one final workgroup
// A pivot that is not positive (non-finite factors) becomes NaN and the NaN spreads through that module's block: nothing
// loops on data, nothing faults.  No atomics; every sum has a fixed order, so identical calls are bit-identical.

namespace dqmc {

// the matrix (2 * module + is_g) that holds element e of the state's matrix part
__device__ inline int kf_find(const long* __restrict__ start, int n_mat, long e) {
  int lo = 0, hi = n_mat;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// ema old + (1 - ema) new with both products rounded before the sum, as the tree path's torch expression: contracted into an
// fma the result differs in the last bits, which shows where old and new nearly cancel
__device__ inline double kf_mix(double old, double nw, double ema) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double a = ema * old, b = (1.0 - ema) * nw;
  return a + b;
}

template <typename real>
__global__ void __launch_bounds__(OPT_BLOCK) k_kf_count(const real* __restrict__ lp, const int32_t* __restrict__ sg, int B,
                                                        double* __restrict__ scal) {
  __shared__ int red[OPT_BLOCK];
  const int tid = threadIdx.x;
  int c = 0;
  for (int b = tid; b < B; b += OPT_BLOCK) {
    const double l = (double)lp[b];
    c += (sg[b] != 0 && l - l == 0) ? 1 : 0;
  }
  red[tid] = c;
  __syncthreads();
  for (int s = OPT_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) scal[0] = (double)(red[0] > 1 ? red[0] : 1);
}

__global__ void __launch_bounds__(OPT_BLOCK) k_kf_assemble(KfTables t, const double* __restrict__ factors, const double* __restrict__ scal,
                                                           double* __restrict__ state, int first, double ema) {
  const double nv = scal[0];
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < t.n_mat_elems; e += (long)gridDim.x * OPT_BLOCK) {
    const int q = kf_find(t.mat_start, 2 * t.n_mod, e);
    const KfMod m = t.mod[q >> 1];
    const int is_g = q & 1, n = is_g ? m.dg : m.da;
    const long rel = e - t.mat_start[q];
    const int i = (int)(rel / n), j = (int)(rel % n);
    double s = 0.0;
    for (int o = m.op0; o < m.op1; ++o) {
      const KfOp op = t.op[o];
      const int32_t* inv = t.inv + (is_g ? op.inv_col : op.inv_row);
      const int d = is_g ? op.d_g : op.d_a;
      s += factors[(is_g ? op.g_off : op.a_off) + (long)inv[i] * d + inv[j]];
    }
    const double f_new = s / (is_g ? nv : nv * (double)m.R);
    state[e] = first ? f_new : kf_mix(state[e], f_new, ema);
  }
}

template <typename real>
__global__ void __launch_bounds__(256) k_kf_diag(KfTables t, const real* __restrict__ rest, long n_rest, int B,
                                                 const double* __restrict__ scal, const double* __restrict__ g,
                                                 double* __restrict__ state_diag, int first, double ema, double damping,
                                                 double* __restrict__ delta, const double* __restrict__ nuc_F) {
  __shared__ double red[4][64];
  const int le = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long e = (long)blockIdx.x * 64 + le;
  double s = 0.0;
  if (e < t.n_diag) {
    const long c0 = t.diag_row[e], c1 = t.diag_row[e + 1];
#pragma unroll 4
    for (int b = q; b < B; b += 4) {
      double o = 0.0;
      for (long c = c0; c < c1; ++c) o += (double)rest[(long)b * n_rest + t.diag_col[c]];
      s += o * o;
    }
    if (nuc_F && c1 == c0) s = q == 0 ? nuc_F[t.diag_pos[e]] : 0.0;      // (the nuclear stream's own parameters: k_nucb_dw summed the squares)
  }
  red[q][le] = s;
  __syncthreads();
  if (q == 0 && e < t.n_diag) {
    const double f_new = (((red[0][le] + red[1][le]) + red[2][le]) + red[3][le]) / scal[0];
    const double f = first ? f_new : kf_mix(state_diag[e], f_new, ema);
    state_diag[e] = f;
    const long pos = t.diag_pos[e];
    delta[pos] = g[pos] / (f + damping);
  }
}

__global__ void __launch_bounds__(64) k_kf_pi(KfTables t, const double* __restrict__ state, double* __restrict__ scal) {
  __shared__ double red[2][64];
  const int tid = threadIdx.x;
  const KfMod m = t.mod[blockIdx.x];
  double a = 0.0, g = 0.0;
  for (int i = tid; i < m.da; i += 64) a += state[m.a_st + (long)i * (m.da + 1)];
  for (int i = tid; i < m.dg; i += 64) g += state[m.g_st + (long)i * (m.dg + 1)];
  red[0][tid] = a; red[1][tid] = g;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) scal[1 + blockIdx.x] = sqrt((red[0][0] / m.da) / (red[1][0] / m.dg));
}

__global__ void __launch_bounds__(OPT_BLOCK) k_kf_load(KfTables t, const double* __restrict__ state, const double* __restrict__ scal,
                                                       double sq, double* __restrict__ M) {
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < t.n_mat_elems; e += (long)gridDim.x * OPT_BLOCK) {
    const int q = kf_find(t.mat_start, 2 * t.n_mod, e);
    const KfMod m = t.mod[q >> 1];
    const int is_g = q & 1, n = is_g ? m.dg : m.da;
    const long rel = e - t.mat_start[q];
    const double pi = scal[1 + (q >> 1)];
    const double damp = is_g ? sq / pi : pi * sq;
    M[e] = state[e] + ((rel / n == rel % n) ? damp : 0.0);
  }
}

// Panel k of every matrix that has one: L_kk = chol(M_kk) in LDS, then L_ik = M_ik L_kk^-T for KF_ROWS rows i per workgroup.
// M is read, L is written: the redundant factorisations of one matrix's workgroups never see each other's stores.
__global__ void __launch_bounds__(KF_ROWS) k_kf_panel(const KfMat* __restrict__ mats, const double* __restrict__ M, double* __restrict__ L,
                                                      int k) {
  __shared__ double Ld[KF_NB][KF_NB + 1];
  __shared__ double tmp[KF_NB];
  const int tid = threadIdx.x;
  const KfMat mt = mats[blockIdx.y];
  const int n = mt.n, j0 = k * KF_NB;
  if (j0 >= n) return;
  const int w = n - j0 < KF_NB ? n - j0 : KF_NB, r0 = j0 + KF_NB;
  const long rb = (long)blockIdx.x * KF_ROWS;
  if (blockIdx.x > 0 && r0 + rb >= n) return;
  const double* Mm = M + mt.ws;
  double* Lm = L + mt.ws;
  for (int e = tid; e < KF_NB * KF_NB; e += KF_ROWS) {
    const int i = e / KF_NB, j = e % KF_NB;
    Ld[i][j] = (i < w && j < w) ? Mm[(long)(j0 + i) * n + j0 + j] : (i == j ? 1.0 : 0.0);      // (identity past a short last panel)
  }
  __syncthreads();
  for (int j = 0; j < KF_NB; ++j) {           // left-looking, column by column; thread i owns row i of the block
    if (tid >= j && tid < KF_NB) {
      double s = Ld[tid][j];
      for (int p = 0; p < j; ++p) s -= Ld[tid][p] * Ld[j][p];
      tmp[tid] = s;
    }
    __syncthreads();
    if (tid >= j && tid < KF_NB) {
      const double piv = tmp[j];
      const double d = piv > 0.0 ? sqrt(piv) : __builtin_nan("");      // not positive or NaN: the block turns NaN
      Ld[tid][j] = tid == j ? d : tmp[tid] / d;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0)
    for (int e = tid; e < KF_NB * KF_NB; e += KF_ROWS) {
      const int i = e / KF_NB, j = e % KF_NB;
      if (i < w && j <= i) Lm[(long)(j0 + i) * n + j0 + j] = Ld[i][j];
    }
  const long r = r0 + rb + tid;
  if (r < n) {                                // (then w == KF_NB)
    double x[KF_NB];
#pragma unroll
    for (int j = 0; j < KF_NB; ++j) x[j] = Mm[r * n + j0 + j];
#pragma unroll
    for (int j = 0; j < KF_NB; ++j) {
      double s = x[j];
#pragma unroll
      for (int p = 0; p < j; ++p) s -= x[p] * Ld[j][p];
      x[j] = s / Ld[j][j];
    }
#pragma unroll
    for (int j = 0; j < KF_NB; ++j) Lm[r * n + j0 + j] = x[j];
  }
}

// M_ij -= sum_p L_ip L_jp over the columns p of panel k, for the lower 16 x 16 tiles (i, j) behind the panel: one per wave
__global__ void __launch_bounds__(256) k_kf_trail(const KfMat* __restrict__ mats, double* __restrict__ M, const double* __restrict__ L,
                                                  int k) {
  const KfMat mt = mats[blockIdx.z];
  const int n = mt.n, j0 = k * KF_NB, r0 = j0 + KF_NB;
  if (r0 >= n) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ti = blockIdx.x, tj = blockIdx.y * 4 + wave;
  const long i0 = r0 + 16L * ti, c0 = r0 + 16L * tj;
  if (i0 >= n || tj > ti) return;             // (a whole wave leaves: the MFMAs below see all 64 lanes or none)
  const double* Lm = L + mt.ws;
  double* Mm = M + mt.ws;
  const long ra = i0 + (lane & 15), rc = c0 + (lane & 15);
  const int kq = lane >> 4;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < KF_NB / 4; ++kk) {
    const int c = j0 + 4 * kk + kq;
    const double a = ra < n ? Lm[ra * n + c] : 0.0;
    const double b = rc < n ? Lm[rc * n + c] : 0.0;
    acc = Mfma<double>::run(a, b, acc);
  }
  const long col = c0 + (lane & 15);
  for (int reg = 0; reg < 4; ++reg) {
    const long row = i0 + Mfma<double>::row_of(lane, reg);
    if (row < n && col < n) Mm[row * n + col] -= acc[reg];
  }
}

// element (i, c) of a module's block [W; b] (da x dg) inside a parameter-ordered vector
__device__ inline long kf_elem(const KfMod& m, int i, int c) {
  return (i < m.n_in ? m.w_pos + (long)i * m.dg : m.b_pos) + c;
}

// X <- X L^-T (backward 0) or X L^-1 (backward 1) for the rows X of one side of every module's block, in place in `x`.
// side 0: L = chol(A_d), row r of X is column r of [W; b]; side 1: L = chol(G_d), row r of X is row r of [W; b].
__global__ void __launch_bounds__(256) k_kf_solve(KfTables t, const double* __restrict__ L, double* x, int side, int backward) {
  __shared__ double Ld[KF_NB][KF_NB + 1];
  __shared__ double T[KF_RB][KF_NB + 1];
  const int tid = threadIdx.x;
  const KfMod m = t.mod[blockIdx.y];
  const int n = side ? m.dg : m.da, nrows = side ? m.da : m.dg;
  const int row0 = blockIdx.x * KF_RB;
  if (row0 >= nrows) return;
  const double* Lm = L + (side ? m.g_st : m.a_st);
  const int jj = tid % KF_NB, rs = tid / KF_NB;
  constexpr int RS = 256 / KF_NB, RQ = KF_RB / RS;      // row slices of the workgroup, rows per thread
  static_assert(RS * KF_NB == 256 && RQ * RS == KF_RB && KF_NB % 4 == 0 && KF_NB <= KF_ROWS, "tiling of the KFAC solve kernels");
  const int nblk = (n + KF_NB - 1) / KF_NB;
  for (int s = 0; s < nblk; ++s) {
    const int kb = backward ? nblk - 1 - s : s, j0 = kb * KF_NB;
    const int w = n - j0 < KF_NB ? n - j0 : KF_NB, j = j0 + jj;
    double acc[RQ];
    long at[RQ];
    for (int q = 0; q < RQ; ++q) {
      const int wr = row0 + rs + RS * q;
      const bool on = wr < nrows && jj < w;
      at[q] = on ? (side ? kf_elem(m, wr, j) : kf_elem(m, j, wr)) : -1;
      acc[q] = on ? x[at[q]] : 0.0;
    }
    if (jj < w) {
      const int p0 = backward ? j0 + w : 0, p1 = backward ? n : j0;
#pragma unroll 4
      for (int p = p0; p < p1; ++p) {          // (unrolled so that several loads are in flight: the loop is bound by their latency)
        const double lv = backward ? Lm[(long)p * n + j] : Lm[(long)j * n + p];
        for (int q = 0; q < RQ; ++q) {
          const int wr = row0 + rs + RS * q;
          if (wr < nrows) acc[q] -= x[side ? kf_elem(m, wr, p) : kf_elem(m, p, wr)] * lv;
        }
      }
    }
    for (int e = tid; e < KF_NB * KF_NB; e += 256) {
      const int i = e / KF_NB, c = e % KF_NB;
      Ld[i][c] = (i < w && c <= i) ? Lm[(long)(j0 + i) * n + j0 + c] : (i == c ? 1.0 : 0.0);
    }
    for (int q = 0; q < RQ; ++q) T[rs + RS * q][jj] = acc[q];
    __syncthreads();
    if (tid < KF_RB && row0 + tid < nrows) {
      if (!backward) {
        for (int a = 0; a < w; ++a) {
          double v = T[tid][a];
          for (int p = 0; p < a; ++p) v -= T[tid][p] * Ld[a][p];
          T[tid][a] = v / Ld[a][a];
        }
      } else {
        for (int a = w - 1; a >= 0; --a) {
          double v = T[tid][a];
          for (int p = a + 1; p < w; ++p) v -= T[tid][p] * Ld[p][a];
          T[tid][a] = v / Ld[a][a];
        }
      }
    }
    __syncthreads();
    for (int q = 0; q < RQ; ++q)
      if (at[q] >= 0) x[at[q]] = T[rs + RS * q][jj];
    __syncthreads();                           // (the next block's dot products read these rows from global memory)
  }
}

__global__ void __launch_bounds__(OPT_BLOCK) k_kf_dot(const double* __restrict__ a, const double* __restrict__ b, long n,
                                                      double* __restrict__ part) {
  double s = 0.0;
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * OPT_BLOCK) s += a[e] * b[e];
  opt_block_sums(s, 0.0, 0.0, part);
}
__global__ void __launch_bounds__(OPT_BLOCK) k_kf_dot_final(const double* __restrict__ part, int nb, double* __restrict__ dot) {
  __shared__ double red[OPT_BLOCK];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int b = tid; b < nb; b += OPT_BLOCK) s += part[b];
  red[tid] = s;
  __syncthreads();
  for (int h = OPT_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) dot[0] = red[0];
}

// theta += -lr coeff delta with kfac_jax's norm constraint (momentum 0) read from device memory
__global__ void __launch_bounds__(OPT_BLOCK) k_kf_apply(double* __restrict__ theta, const double* __restrict__ delta,
                                                        const double* __restrict__ dot, double lr, double norm_constraint, long n,
                                                        double* __restrict__ part) {
  const double d = dot[0];
  double coeff = 1.0;
  if (norm_constraint > 0.0 && d > 0.0) {
    coeff = sqrt(norm_constraint / (lr * lr * d));
    if (coeff > 1.0) coeff = 1.0;
  }
  const double scale = -lr * coeff;
  double sp = 0, sg = 0, su = 0;
  for (long e = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * OPT_BLOCK) {
    const double de = delta[e], th = theta[e], upd = scale * de;
    theta[e] = th + upd;
    sp += th * th; sg += de * de; su += upd * upd;
  }
  if (part) opt_block_sums(sp, sg, su, part);
}
__global__ void __launch_bounds__(OPT_BLOCK) k_kf_norms4(const double* __restrict__ part, int nb, const double* __restrict__ dot,
                                                         double lr, double* __restrict__ norms4) {
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
  if (tid < 3) norms4[tid] = sqrt(red[tid][0]);
  if (tid == 3) norms4[3] = lr * lr * dot[0];
}

template <typename real>
void launch_kfac_direction(hipStream_t st, const KfacDirArgs& a) {
  const KfTables& t = a.t;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kf_count<real>), dim3(1), dim3(OPT_BLOCK), 0, st, (const real*)a.logpsi, a.sign, a.B, a.scal);
  if (t.n_diag > 0)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kf_diag<real>), dim3((unsigned)((t.n_diag + 63) / 64)), dim3(256), 0, st, t, (const real*)a.rest,
                       a.n_rest, a.B, (const double*)a.scal, a.g, a.state + t.n_mat_elems, a.first, a.ema, a.damping, a.delta, a.nuc_F);
  if (t.n_mod > 0) {
    const int ng = opt_grid(t.n_mat_elems);
    hipLaunchKernelGGL(k_kf_assemble, dim3(ng), dim3(OPT_BLOCK), 0, st, t, a.factors, (const double*)a.scal, a.state, a.first, a.ema);
    hipLaunchKernelGGL(k_kf_pi, dim3(t.n_mod), dim3(64), 0, st, t, (const double*)a.state, a.scal);
    hipLaunchKernelGGL(k_kf_load, dim3(ng), dim3(OPT_BLOCK), 0, st, t, (const double*)a.state, (const double*)a.scal, sqrt(a.damping), a.M);
    for (int k = 0; k < a.n_panels; ++k) {
      const int left = a.max_n - (k + 1) * KF_NB;      // rows of the largest matrix behind panel k
      const int rblocks = left > 0 ? (left + KF_ROWS - 1) / KF_ROWS : 1;
      hipLaunchKernelGGL(k_kf_panel, dim3(rblocks, a.active[k]), dim3(KF_ROWS), 0, st, t.mats, (const double*)a.M, a.L, k);
      if (left > 0) {
        const int nt = (left + 15) / 16;
        hipLaunchKernelGGL(k_kf_trail, dim3(nt, (nt + 3) / 4, a.active[k + 1]), dim3(256), 0, st, t.mats, a.M, (const double*)a.L, k);
      }
    }
    for (int step = 0; step < 4; ++step) {             // A^-1 from the left (side 0), then G^-1 from the right (side 1)
      const int side = step >> 1, nrows = side ? a.max_da : a.max_dg;
      hipLaunchKernelGGL(k_kf_solve, dim3((nrows + KF_RB - 1) / KF_RB, t.n_mod), dim3(256), 0, st, t, (const double*)a.L, a.delta, side,
                         step & 1);
    }
  }
  const int nb = opt_grid(a.n_params);
  hipLaunchKernelGGL(k_kf_dot, dim3(nb), dim3(OPT_BLOCK), 0, st, (const double*)a.delta, a.g, a.n_params, a.part);
  hipLaunchKernelGGL(k_kf_dot_final, dim3(1), dim3(OPT_BLOCK), 0, st, (const double*)a.part, nb, a.dot);
}

void launch_kfac_apply(hipStream_t st, double* theta, const double* delta, const double* dot, double lr, double norm_constraint, long n,
                       double* part, double* norms4) {
  const int nb = opt_grid(n);
  hipLaunchKernelGGL(k_kf_apply, dim3(nb), dim3(OPT_BLOCK), 0, st, theta, delta, dot, lr, norm_constraint, n, norms4 ? part : nullptr);
  if (norms4) hipLaunchKernelGGL(k_kf_norms4, dim3(1), dim3(OPT_BLOCK), 0, st, (const double*)part, nb, dot, lr, norms4);
}

template void launch_kfac_direction<float>(hipStream_t, const KfacDirArgs&);
template void launch_kfac_direction<double>(hipStream_t, const KfacDirArgs&);

}  // namespace dqmc
