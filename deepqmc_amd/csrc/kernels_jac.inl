// kernels_jac.inl -- per-walker parameter Jacobian of log|psi| (dqmc_log_psi_jacobian).  Included by kernel_linear.hip after
// kernels_grad.inl, whose k_lin_dz / k_lin_dz_rowsum / k_lin_dx it reuses.
//
// Row b of J is the gradient of log|psi(r_b)| over the flat weight buffer.  Per walker and per LINEAR piece that is one
// contiguous block of pad4(K) * ldw entries of the row (the outer products of the piece's inputs with dZ, summed over
// the walker's rows), so the kernel is a store stream: each workgroup forms a tile of at most JAC_TILE entries of one
// walker's block in registers (4 x 4 outputs per thread, the walker's rows summed in order), stages it in LDS and writes it
// back as 16-byte stores by consecutive lanes (1 KiB per wave instruction).  One owner per entry, no atomics.
// A walker whose sign is 0 or whose log|psi| is not finite gets zeros, whatever its adjoints hold.

namespace dqmc {

template <typename real> struct JacVec;
template <> struct JacVec<float> { typedef float t __attribute__((vector_size(16))); static constexpr int n = 4; };
template <> struct JacVec<double> { typedef double t __attribute__((vector_size(16))); static constexpr int n = 2; };

template <typename real>
__device__ __forceinline__ bool jac_bad_walker(const real* lp, const int32_t* sg, long b) {
  const double l = (double)lp[b];
  return sg[b] == 0 || !(l - l == 0);
}

// J[b][col + (kk0 + r) * ldw + n0 + c] (=, or += with accum) sum_rr x[b, rr, kk0 + r] dZ[b, rr, n0 + c] over the tile rows
// r < min(tr, rows_blk - kk0) and columns c < min(nc, ldw - n0); x = X[b * rpw + r0 + (bcast ? 0 : rr)][kk] for kk < K and 0
// beyond (X == nullptr: a row of ones, the bias block).  Grid: (walker, row tile, column tile).
template <typename real>
__global__ void __launch_bounds__(256) k_lin_jac(const real* __restrict__ X, int ld, int rpw, int r0, int bcast, int K, int rows_blk,
                                                 const real* __restrict__ dZ, int nrows, int ldw, int tr, int nc,
                                                 const real* __restrict__ lp, const int32_t* __restrict__ sg, real* __restrict__ J,
                                                 long ld_jac, long col, int accum, int vec) {
  __shared__ real tile[JAC_TILE];
  const long b = blockIdx.x;
  const int kk0 = blockIdx.y * tr, n0 = blockIdx.z * nc;
  const int rows = rows_blk - kk0 < tr ? rows_blk - kk0 : tr;
  const int cols = ldw - n0 < nc ? ldw - n0 : nc;          // a multiple of 4 (ldw and nc are)
  const int t = threadIdx.x;
  const bool bad = jac_bad_walker(lp, sg, b);
  if (!bad) {
    const int cq = cols >> 2, nq = ((rows + 3) >> 2) * cq;
    for (int q = t; q < nq; q += 256) {
      const int kq = (q / cq) * 4, n4 = (q - (q / cq) * cq) * 4;
      real acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
      const real* zr = dZ + (long)b * nrows * ldw + n0 + n4;
      for (int rr = 0; rr < nrows; ++rr) {
        real x[4], z[4];
        const real* xr = X ? X + ((long)b * rpw + r0 + (bcast ? 0 : rr)) * ld : nullptr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kk = kk0 + kq + i;
          x[i] = kk < K ? (xr ? xr[kk] : (real)1) : (real)0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = zr[(long)rr * ldw + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += x[i] * z[j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (kq + i < rows)
#pragma unroll
          for (int j = 0; j < 4; ++j) tile[(kq + i) * cols + n4 + j] = acc[i][j];
    }
  }
  __syncthreads();
  real* dst = J + b * ld_jac + col + (long)kk0 * ldw + n0;
  const int n_el = rows * cols;
  if (vec) {
    typedef typename JacVec<real>::t vt;
    constexpr int V = JacVec<real>::n;
    for (int e = t * V; e < n_el; e += 256 * V) {
      const int r = e / cols, c = e - r * cols;
      vt v;
#pragma unroll
      for (int u = 0; u < V; ++u) v[u] = bad ? (real)0 : tile[e + u];
      vt* p = reinterpret_cast<vt*>(dst + (long)r * ldw + c);
      if (accum && !bad) v += *p;
      *p = v;
    }
  } else {
    for (int e = t; e < n_el; e += 256) {
      const int r = e / cols, c = e - r * cols;
      real* p = dst + (long)r * ldw + c;
      const real v = bad ? (real)0 : tile[e];
      *p = accum && !bad ? *p + v : v;
    }
  }
}

// J[b][col + m] (= or +=) (real) src[b * stride + m] for m < n: the per-walker partials of CONST, ORBITALS and FINAL
template <typename T, typename real>
__global__ void __launch_bounds__(256) k_jac_scatter(const T* __restrict__ src, long stride, int n, const real* __restrict__ lp,
                                                     const int32_t* __restrict__ sg, real* __restrict__ J, long ld_jac, long col,
                                                     int accum, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n;
  const int m = (int)(idx - b * n);
  real* p = J + b * ld_jac + col + m;
  if (jac_bad_walker(lp, sg, b)) { *p = 0; return; }
  const real v = (real)src[b * stride + m];
  *p = accum ? *p + v : v;
}

// J[b][cols[m]] = 0 for m < n (cols == nullptr: the columns 0 .. n-1)
template <typename real>
__global__ void __launch_bounds__(256) k_jac_zero(real* __restrict__ J, long ld_jac, const int32_t* __restrict__ cols, int n, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n;
  const int m = (int)(idx - b * n);
  J[b * ld_jac + (cols ? cols[m] : m)] = 0;
}

// ---- launchers ----

template <typename real>
static void jac_block(hipStream_t st, const real* X, int ld, int rpw, int r0, int bcast, int K, int rows_blk, const real* dZ, int nrows,
                      int ldw, int B, const JacOut<real>& o, long col) {
  const int nc = ldw < JAC_MAX_COLS ? ldw : JAC_MAX_COLS;
  int tr = JAC_TILE / nc / 4 * 4;
  if (tr > rows_blk) tr = rows_blk;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_jac<real>), dim3((unsigned)B, (unsigned)((rows_blk + tr - 1) / tr), (unsigned)((ldw + nc - 1) / nc)),
                     dim3(256), 0, st, X, ld, rpw, r0, bcast, K, rows_blk, dZ, nrows, ldw, tr, nc, o.lp, o.sg, o.J, o.ld, col,
                     o.accum, o.vec);
}

template <typename real>
void launch_linear_jac(hipStream_t st, const LinBwdArgs<real>& a, const JacOut<real>& o, long w_col, long bias_col) {
  const long M = (long)a.B * a.nrows, nz = M * a.ldw;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dz<real>), dim3(grad_grid(nz)), dim3(256), 0, st, a.Z, a.dZ, a.dY, a.ld_dst, a.rpw_dst,
                     a.r0_dst, a.col0_dst, a.dres, a.ld_res, a.rpw_res, a.r0_res, a.dres ? a.res_scale : (real)1, a.act, a.nrows,
                     a.nout, a.ldw, nz);
  if (bias_col >= 0) jac_block<real>(st, nullptr, 0, 1, 0, 0, 1, 1, a.dZ, a.nrows, a.ldw, a.B, o, bias_col);
  bool have_rowsum = false;
  for (int p = 0; p < a.n_pieces; ++p) {
    const LinBwdPiece<real>& q = a.piece[p];
    const int kt = (q.K + 15) / 16, Kp = (q.K + 3) / 4 * 4;
    const long col = w_col + (long)q.w_row * a.ldw;
    if (q.bcast && !have_rowsum) {      // a broadcast piece sees the per-walker sum of the segment's rows of dZ
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dz_rowsum<real>), dim3(grad_grid((long)a.B * a.ldw)), dim3(256), 0, st,
                         (const real*)a.dZ, a.dZs, a.nrows, a.ldw, (long)a.B * a.ldw);
      have_rowsum = true;
    }
    if (q.bcast) jac_block<real>(st, q.X, q.ld, q.rpw, q.r0, 1, q.K, Kp, a.dZs, 1, a.ldw, a.B, o, col);
    else jac_block<real>(st, q.X, q.ld, q.rpw, q.r0, 0, q.K, Kp, a.dZ, a.nrows, a.ldw, a.B, o, col);
    if (!q.dX) continue;
    if (q.bcast)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dx<real>), dim3((unsigned)((a.B + 63) / 64), (unsigned)kt), dim3(256), 0, st,
                         (const real*)a.dZs, 1, (long)a.B, a.W, a.ldw, q.w_row, q.K, q.dX, q.ld, q.rpw, q.r0);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dx<real>), dim3((unsigned)((M + 63) / 64), (unsigned)kt), dim3(256), 0, st,
                         (const real*)a.dZ, a.nrows, M, a.W, a.ldw, q.w_row, q.K, q.dX, q.ld, q.rpw, q.r0);
  }
}

template <typename T, typename real>
void launch_jac_scatter(hipStream_t st, const T* src, long stride, int n, int B, const JacOut<real>& o, long col) {
  const long total = (long)B * n;
  if (n > 0)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_scatter<T, real>), dim3(grad_grid(total)), dim3(256), 0, st, src, stride, n, o.lp, o.sg, o.J,
                       o.ld, col, o.accum, total);
}

template <typename real>
void launch_jac_zero(hipStream_t st, real* J, long ld_jac, const int32_t* cols, int n, int B) {
  const long total = (long)B * n;
  if (n > 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_zero<real>), dim3(grad_grid(total)), dim3(256), 0, st, J, ld_jac, cols, n, total);
}

#define DQMC_JAC_INST(real)                                                                                                         \
  template void launch_linear_jac<real>(hipStream_t, const LinBwdArgs<real>&, const JacOut<real>&, long, long);                   \
  template void launch_jac_scatter<real, real>(hipStream_t, const real*, long, int, int, const JacOut<real>&, long);               \
  template void launch_jac_zero<real>(hipStream_t, real*, long, const int32_t*, int, int);
DQMC_JAC_INST(float)
DQMC_JAC_INST(double)
#undef DQMC_JAC_INST
template void launch_jac_scatter<double, float>(hipStream_t, const double*, long, int, int, const JacOut<float>&, long);

}  // namespace dqmc
