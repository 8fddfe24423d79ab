// kernels_kfac.inl -- KFAC Kronecker factors of the LINEAR ops (dqmc_log_psi_kfac).  Included by kernel_linear.hip after
// kernels_grad.inl, whose reverse pass forms the pre-activation adjoint dZ these kernels read.
//
// Both factors of an op are Gram matrices C = sum_m y_m y_m^T over the M = B * nrows rows of a walker chunk: y = the op's
// input row (the virtual concatenation of its pieces, zero padded to pad4(K) each, plus a trailing 1 for the bias) for A,
// y = dZ for G.  k_kfac_gram splits the rows over gridDim.y and the upper triangle into 64 x 128-column super-tiles over
// gridDim.x; a workgroup stages a block of rows of its columns in LDS once and its four waves form eight 16 x 16 tiles each
// from it with 16x16x4 MFMAs, accumulating over the split in registers; each split writes its tiles as double partials.
// k_kfac_reduce sums the partials of every entry in split order and mirrors the upper triangle.  Walkers whose validity flag
// is 0 contribute exact zeros.  No atomics anywhere.

namespace dqmc {

// Column descriptor of y: piece p and entry kk of column c, -1 = zero (padding, past D), -2 = the bias 1
template <typename real>
__device__ __forceinline__ void gram_col(const GramArgs<real>& g, int c, int& p, int& kk) {
  p = -1; kk = 0;
  if (c >= g.D) return;
  if (c == g.bias_col) { p = -2; return; }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q >= g.n_pieces) break;
    const int k = c - g.piece[q].col0;
    if (k >= 0 && k < g.piece[q].Kp) {
      if (k < g.piece[q].K) { p = q; kk = k; }
      return;
    }
  }
}

template <typename real>
__device__ __forceinline__ real gram_load(const GramArgs<real>& g, int p, int kk, long b, int rr) {
  if (p == -2) return (real)1;
  if (p < 0) return (real)0;
  const GramPiece<real>& q = g.piece[p];
  return q.X[(b * q.rpw + q.r0 + (q.bcast ? 0 : rr)) * q.ld + kk];
}

// part[s][t][16][16]: split s's sum over its rows of the upper-triangular tile t = (ti, tj), ti <= tj, row-major over the
// upper triangle of the nt x nt tile grid.  Grid: (super-tiles, splits), 256 threads.  A super-tile is GRAM_TI x GRAM_TJ
// tiles: columns [64 I, 64 I + 64) against [128 J, 128 J + 128), only those with a tile on or above the diagonal; wave w
// owns tile row 4 I + w and its eight tiles share one A operand.  A workgroup stages RB rows of its 64 + 128 columns in LDS
// (row pitches 80 and 144 entries, = 16 mod 32: the four rows one MFMA operand read touches fall in distinct bank groups),
// then forms its tiles from LDS with 16x16x4 MFMAs, accumulating over its split in registers.
template <typename real>
__global__ void __launch_bounds__(256) k_kfac_gram(GramArgs<real> g, int nt, int T, long m_per, int RB, double* __restrict__ part) {
  typedef typename Mfma<real>::acc_t acc_t;
  constexpr int PI = GRAM_TI * 16 + 16, PJ = GRAM_TJ * 16 + 16, RBA = sizeof(real) == 4 ? GRAM_RB_MAX : GRAM_RB_MAX / 2;
  __shared__ real yi[RBA * PI];                      // 56 KiB in float and in double
  __shared__ real yj[RBA * PJ];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = blockIdx.y;
  // super-tile (I, J) of this workgroup: the upper ones in row-major order
  const int nJ = (nt + GRAM_TJ - 1) / GRAM_TJ;
  int I = 0, J = 0;
  {
    int rem = blockIdx.x;
    for (;; ++I) {
      const int j0 = (GRAM_TI * I - (GRAM_TJ - 1)) > 0 ? (GRAM_TI * I - (GRAM_TJ - 1) + GRAM_TJ - 1) / GRAM_TJ : 0;
      if (rem < nJ - j0) { J = j0 + rem; break; }
      rem -= nJ - j0;
    }
  }
  const int ti = GRAM_TI * I + wv;
  const long m_beg = (long)s * m_per;
  const long m_end = m_beg + m_per < g.M ? m_beg + m_per : g.M;
  // staging: lane covers column lane of the I block and columns lane, lane + 64 of the J block, the wave every 4th row
  int pc[3], kc[3];
  gram_col<real>(g, GRAM_TI * 16 * I + lane, pc[0], kc[0]);
  gram_col<real>(g, GRAM_TJ * 16 * J + lane, pc[1], kc[1]);
  gram_col<real>(g, GRAM_TJ * 16 * J + 64 + lane, pc[2], kc[2]);
  acc_t acc[GRAM_TJ];
#pragma unroll
  for (int u = 0; u < GRAM_TJ; ++u) acc[u] = acc_t{0, 0, 0, 0};
  bool live[GRAM_TJ];
#pragma unroll
  for (int u = 0; u < GRAM_TJ; ++u) { const int tj = GRAM_TJ * J + u; live[u] = ti < nt && tj < nt && ti <= tj; }
  const int c16 = lane & 15, k4 = lane >> 4;
  for (long mb = m_beg; mb < m_end; mb += RB) {
    const int nb = m_end - mb < RB ? (int)(m_end - mb) : RB;
    __syncthreads();
    for (int row = wv; row < RB; row += 4) {
      real v0 = 0, v1 = 0, v2 = 0;
      if (row < nb) {
        const long m = mb + row;
        const long b = m / g.nrows;
        const int rr = (int)(m - b * g.nrows);
        if (g.ok[b] != 0) {
          v0 = gram_load<real>(g, pc[0], kc[0], b, rr);
          v1 = gram_load<real>(g, pc[1], kc[1], b, rr);
          v2 = gram_load<real>(g, pc[2], kc[2], b, rr);
        }
      }
      yi[row * PI + lane] = v0;
      yj[row * PJ + lane] = v1;
      yj[row * PJ + 64 + lane] = v2;
    }
    __syncthreads();
    const int nb4 = (nb + 3) & ~3;                    // rows nb .. nb4 - 1 hold zeros
    if (ti < nt)
      for (int r0 = 0; r0 < nb4; r0 += 4) {
        const real a = yi[(r0 + k4) * PI + wv * 16 + c16];
        const real* yr = yj + (r0 + k4) * PJ + c16;
#pragma unroll
        for (int u = 0; u < GRAM_TJ; ++u)
          if (live[u]) acc[u] = Mfma<real>::run(a, yr[u * 16], acc[u]);
      }
  }
#pragma unroll
  for (int u = 0; u < GRAM_TJ; ++u)
    if (live[u]) {
      const int tj = GRAM_TJ * J + u;
      const long t = (long)ti * nt - (long)ti * (ti - 1) / 2 + (tj - ti);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        part[((long)s * T + t) * 256 + Mfma<real>::row_of(lane, j) * 16 + c16] = (double)acc[u][j];
    }
}

// out[i][j] += sum_s part[s][tile(lo, hi)][lo % 16][hi % 16], lo = min(i, j), hi = max(i, j): both triangles read the one
// upper-triangular entry, so the result is exactly symmetric
__global__ void __launch_bounds__(256) k_kfac_reduce(const double* __restrict__ part, int S, int T, int nt, int D, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)D * D) return;
  const int i = (int)(idx / D), j = (int)(idx - (long)i * D);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const int a = lo >> 4, c = hi >> 4;
  const long t = (long)a * nt - (long)a * (a - 1) / 2 + (c - a);
  const double* p = part + t * 256 + (lo & 15) * 16 + (hi & 15);
  double sum = 0;
  for (int q = 0; q < S; ++q) sum += p[(long)q * T * 256];
  out[idx] += sum;
}

// per-walker weights of one chunk: w[b] = cot[b] (1 without a cotangent) and w[B + b] = 1 for a valid walker, both 0 for a
// walker whose sign is 0 or whose log|psi| is not finite
template <typename real>
__global__ void __launch_bounds__(256) k_kfac_weights(const real* __restrict__ lp, const int32_t* __restrict__ sg,
                                                      const real* __restrict__ cot, double* __restrict__ w, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double l = (double)lp[b];
  const bool ok = sg[b] != 0 && l - l == 0;
  w[b] = ok ? (cot ? (double)cot[b] : 1.0) : 0.0;
  w[B + b] = ok ? 1.0 : 0.0;
}

// ---- launchers ----

// tiles, tile groups and splits of one Gram product of D columns over M rows (the same on the host for the workspace bound)
static long gram_supertiles(int nt) {
  const int nI = (nt + GRAM_TI - 1) / GRAM_TI, nJ = (nt + GRAM_TJ - 1) / GRAM_TJ;
  long n = 0;
  for (int I = 0; I < nI; ++I) {
    const int j0 = (GRAM_TI * I - (GRAM_TJ - 1)) > 0 ? (GRAM_TI * I - (GRAM_TJ - 1) + GRAM_TJ - 1) / GRAM_TJ : 0;
    n += nJ - j0;
  }
  return n;
}
GramPlan gram_plan(int D, long M, int real_bytes) {
  GramPlan p{};
  p.nt = (D + 15) / 16;
  p.T = p.nt * (p.nt + 1) / 2;
  p.RB = real_bytes == 4 ? GRAM_RB_MAX : GRAM_RB_MAX / 2;
  p.groups = gram_supertiles(p.nt);
  long S = (GRAM_WGS + p.groups - 1) / p.groups;
  const long cap = (M + p.RB - 1) / p.RB;
  if (S > cap) S = cap;
  if (S < 1) S = 1;
  p.m_per = ((M + S - 1) / S + 3) / 4 * 4;
  if (p.m_per < 4) p.m_per = 4;
  p.S = (M + p.m_per - 1) / p.m_per;
  if (p.S < 1) p.S = 1;
  return p;
}
size_t gram_part_doubles(int D) {       // largest part[] of a D-column product, any M
  const int nt = (D + 15) / 16, T = nt * (nt + 1) / 2;
  const long groups = gram_supertiles(nt);
  return (size_t)((GRAM_WGS + groups - 1) / groups) * T * 256;
}

template <typename real>
void launch_kfac_gram(hipStream_t st, const GramArgs<real>& g, double* out, double* part) {
  const GramPlan p = gram_plan(g.D, g.M, (int)sizeof(real));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kfac_gram<real>), dim3((unsigned)p.groups, (unsigned)p.S), dim3(256), 0, st, g, p.nt, p.T,
                     p.m_per, p.RB, part);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kfac_reduce), dim3(grad_grid((long)g.D * g.D)), dim3(256), 0, st, (const double*)part, (int)p.S,
                     p.T, p.nt, g.D, out);
}

template <typename real>
void launch_kfac_factors(hipStream_t st, const LinBwdArgs<real>& a, int has_bias, const double* ok, double* A, double* G, double* part) {
  GramArgs<real> g{};
  g.n_pieces = a.n_pieces;
  int col = 0;
  for (int p = 0; p < a.n_pieces; ++p) {
    const LinBwdPiece<real>& q = a.piece[p];
    g.piece[p] = GramPiece<real>{q.X, q.ld, q.rpw, q.r0, q.K, (q.K + 3) / 4 * 4, q.bcast, col};
    col += (q.K + 3) / 4 * 4;
  }
  g.bias_col = has_bias ? col : -1;
  g.D = col + (has_bias ? 1 : 0);
  g.nrows = a.nrows; g.M = (long)a.B * a.nrows; g.ok = ok;
  launch_kfac_gram<real>(st, g, A, part);
  GramArgs<real> h{};
  h.n_pieces = 1;
  h.piece[0] = GramPiece<real>{a.dZ, a.ldw, a.nrows, 0, a.ldw, a.ldw, 0, 0};
  h.bias_col = -1;
  h.D = a.ldw;
  h.nrows = a.nrows; h.M = g.M; h.ok = ok;
  launch_kfac_gram<real>(st, h, G, part);
}

template <typename real>
void launch_kfac_weights(hipStream_t st, const real* lp, const int32_t* sg, const real* cot, double* w, int B) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kfac_weights<real>), dim3(grad_grid(B)), dim3(256), 0, st, lp, sg, cot, w, B);
}

#define DQMC_KFAC_INST(real)                                                                                                        \
  template void launch_kfac_factors<real>(hipStream_t, const LinBwdArgs<real>&, int, const double*, double*, double*, double*);   \
  template void launch_kfac_weights<real>(hipStream_t, const real*, const int32_t*, const real*, double*, int);
DQMC_KFAC_INST(float)
DQMC_KFAC_INST(double)
#undef DQMC_KFAC_INST

}  // namespace dqmc
