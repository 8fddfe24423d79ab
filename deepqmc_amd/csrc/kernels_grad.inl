// kernels_grad.inl -- reverse pass of the value-only layer program (TP = 1): the parameter gradient of log|psi|
// contracted with a cotangent per walker (dqmc_log_psi_vjp).  Included by kernel_linear.hip (it needs act_derivs).
//
// Layouts are those of the value pass: activation buffer b is real[B][rows][width]; its adjoint has the same shape.
// Every kernel here owns the adjoint elements it writes (one thread per element, gathers through host-built tables),
// and every walker-reduced parameter gradient is summed in a fixed order (per-walker or per-split partials, then a
// second pass), so two identical calls give bit-identical gradients: no floating-point atomics anywhere.

namespace dqmc {

// ---- LINEAR ----

// dZ = (scale dY) * act'(Z) over the B * nrows * ldw pre-activations (columns >= nout: exact zeros); the residual input of
// out = scale (res + y) receives scale dY
template <typename real>
__global__ void __launch_bounds__(256) k_lin_dz(const real* __restrict__ Z, real* __restrict__ dZ, const real* __restrict__ dY,
                                                int ld_dst, int rpw_dst, int r0_dst, int col0, real* __restrict__ dres, int ld_res,
                                                int rpw_res, int r0_res, real scale, int act, int nrows, int nout, int ldw, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx % ldw);
  const long m = idx / ldw;
  const int rr = (int)(m % nrows);
  const long b = m / nrows;
  if (n >= nout) { dZ[idx] = 0; return; }
  real g = dY[(b * rpw_dst + r0_dst + rr) * ld_dst + col0 + n];
  if (dres) {
    dres[(b * rpw_res + r0_res + rr) * ld_res + col0 + n] += scale * g;
    g *= scale;
  }
  real y, d1, d2;
  act_derivs<real>(act, Z[idx], y, d1, d2);
  dZ[idx] = g * d1;
}

// per-walker sum of dZ over the rows of a segment (the adjoint of a broadcast piece collects every destination row)
template <typename real>
__global__ void __launch_bounds__(256) k_lin_dz_rowsum(const real* __restrict__ dZ, real* __restrict__ out, int nrows, int ldw, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx % ldw);
  const long b = idx / ldw;
  real s = 0;
  for (int rr = 0; rr < nrows; ++rr) s += dZ[(b * nrows + rr) * ldw + n];
  out[idx] = s;
}

// dX[m][k] += sum_n dZ[m][n] W[w_row + k][n] for k < K: a 16 x 16 tile (rows m, columns k) per wave, 16x16x4 MFMAs over n.
// Row m = (b, rr) of the segment is row b * rpw + r0 + rr of the source buffer (nrows = 1 for a broadcast piece).
template <typename real>
__global__ void __launch_bounds__(256) k_lin_dx(const real* __restrict__ dZ, int nrows, long M, const real* __restrict__ W, int ldw,
                                                int w_row, int K, real* __restrict__ dX, int ld, int rpw, int r0) {
  typedef typename Mfma<real>::acc_t acc_t;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long m0 = ((long)blockIdx.x * 4 + wv) * 16;
  const int k0 = blockIdx.y * 16;
  const long ma = m0 + (lane & 15);
  const int kb = k0 + (lane & 15);
  acc_t acc = acc_t{0, 0, 0, 0};
  for (int n0 = 0; n0 < ldw; n0 += 4) {
    const int n = n0 + (lane >> 4);
    const real a = ma < M ? dZ[ma * ldw + n] : (real)0;
    const real bv = kb < K ? W[(long)(w_row + kb) * ldw + n] : (real)0;
    acc = Mfma<real>::run(a, bv, acc);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long m = m0 + Mfma<real>::row_of(lane, j);
    if (m < M && kb < K) {
      const long b = m / nrows;
      const int rr = (int)(m - b * nrows);
      dX[(b * rpw + r0 + rr) * ld + kb] += acc[j];
    }
  }
}

// Split-K weight gradient: part[s][kk][n] = sum over the rows m of split s of X[m][kk] dZ[m][n], one 16 x 16 tile per wave
// (X == nullptr: a row of ones, i.e. the bias gradient sum_m dZ[m][n]).
template <typename real>
__global__ void __launch_bounds__(64) k_lin_dw(const real* __restrict__ X, int ld, int rpw, int r0, int bcast, int K,
                                               const real* __restrict__ dZ, int ldw, int nrows, long M, long m_per,
                                               double* __restrict__ part, const double* __restrict__ wt) {
  typedef typename Mfma<real>::acc_t acc_t;
  const int lane = threadIdx.x & 63;
  const int k0 = blockIdx.x * 16, n0 = blockIdx.y * 16, s = blockIdx.z;
  const int Kt = gridDim.x * 16, Nt = gridDim.y * 16;
  const long m_beg = (long)s * m_per;
  const long m_end = m_beg + m_per < M ? m_beg + m_per : M;
  const int kk = k0 + (lane & 15), n = n0 + (lane & 15);
  acc_t acc = acc_t{0, 0, 0, 0};
  for (long mb = m_beg; mb < m_end; mb += 4) {
    const long m = mb + (lane >> 4);
    real a = 0, bv = 0;
    if (m < m_end) {
      const long b = m / nrows;
      const int rr = (int)(m - b * nrows);
      if (kk < K) a = X ? X[(b * rpw + r0 + (bcast ? 0 : rr)) * ld + kk] : (real)1;
      if (n < ldw) bv = dZ[m * ldw + n];
      if (wt) {      // a walker of weight 0 contributes exactly nothing, whatever its inputs hold (a NaN coordinate makes X NaN)
        const double w = wt[b];
        bv = w == 0 ? (real)0 : (real)((double)bv * w);
        if (w == 0) a = 0;
      }
    }
    acc = Mfma<real>::run(a, bv, acc);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) part[((long)s * Kt + k0 + Mfma<real>::row_of(lane, j)) * Nt + n] = (double)acc[j];
}

// fixed-order sum of the split partials into the gradient of the K x nout block (padding rows / columns untouched)
__global__ void __launch_bounds__(256) k_lin_dw_reduce(const double* __restrict__ part, int S, int Kt, int Nt, int K, int nout, int ldw,
                                                       double* __restrict__ g) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= K * nout) return;
  const int kk = idx / nout, n = idx - kk * nout;
  double s = 0;
  for (int q = 0; q < S; ++q) s += part[((long)q * Kt + kk) * Nt + n];
  g[(long)kk * ldw + n] += s;
}

// out[m] += sum_c in[c * stride + m], c < count: one workgroup per m, strided partial sums then a fixed tree
// (wt: term c is in[c * stride + m] * wt[c], exactly 0 where wt[c] == 0)
template <typename T>
__global__ void __launch_bounds__(256) k_colsum(const T* __restrict__ in, long count, long stride, double* __restrict__ out,
                                                const double* __restrict__ wt) {
  __shared__ double red[256];
  const int m = blockIdx.x, t = threadIdx.x;
  double s = 0;
  if (wt) {
    for (long c = t; c < count; c += 256) s += wt[c] == 0 ? 0.0 : (double)in[c * stride + m] * wt[c];
  } else {
    for (long c = t; c < count; c += 256) s += (double)in[c * stride + m];
  }
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) out[m] += red[0];
}

// ---- graph ops ----

template <typename real>
__global__ void __launch_bounds__(256) k_spin_mean_bwd(real* __restrict__ dx, const real* __restrict__ dm, int N, int n_up, int width,
                                                       long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % width);
  const long q = idx / width;
  const int i = (int)(q % N);
  const long b = q / N;
  const int up = i < n_up, cnt = up ? n_up : N - n_up;
  dx[idx] += dm[(b * 2 + (up ? 0 : 1)) * width + c] / (real)cnt;
}

template <typename real>
__global__ void __launch_bounds__(256) k_row_sum_bwd(real* __restrict__ dx, const real* __restrict__ ds, int rows, int width, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % width);
  const long b = idx / ((long)rows * width);
  dx[idx] += ds[b * width + c];
}

// Edge-row adjoint of CONV (hx != nullptr: dwe[row] = sum dout[i] * hx[send]) and EDGE_SUM (hx == nullptr: de[row] = sum dout[i] * scale)
// over the (receiver, sender) pairs that read edge row `row`: rtab[row][Sr][2], receiver -1 = none.
template <typename real>
__global__ void __launch_bounds__(256) k_edge_rows_bwd(real* __restrict__ dwe, int we_rows, int we_w, const real* __restrict__ hx,
                                                       int hx_rows, int hx_w, const real* __restrict__ dout, int out_w, int col0,
                                                       const int32_t* __restrict__ rtab, int Sr, int W, int N, real scale, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % W);
  const long q = idx / W;
  const int row = (int)(q % we_rows);
  const long b = q / we_rows;
  real s = 0;
  for (int e = 0; e < Sr; ++e) {
    const int i = rtab[(row * Sr + e) * 2], snd = rtab[(row * Sr + e) * 2 + 1];
    if (i < 0) continue;
    const real g = dout[(b * N + i) * out_w + col0 + c];
    s += hx ? g * hx[(b * hx_rows + (snd >= 0 ? snd : -1 - snd)) * hx_w + c] : g * scale;
  }
  dwe[(b * we_rows + row) * we_w + c] += s;
}

// Sender adjoint of CONV: dhx[srow] = sum over (receiver i, edge row) with that sender of dout[i] * we[row]; stab[srow][Ss][2]
template <typename real>
__global__ void __launch_bounds__(256) k_conv_send_bwd(real* __restrict__ dhx, int hx_rows, int hx_w, const real* __restrict__ we,
                                                       int we_rows, int we_w, const real* __restrict__ dout, int out_w, int col0,
                                                       const int32_t* __restrict__ stab, int Ss, int W, int N, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % W);
  const long q = idx / W;
  const int srow = (int)(q % hx_rows);
  const long b = q / hx_rows;
  real s = 0;
  for (int e = 0; e < Ss; ++e) {
    const int i = stab[(srow * Ss + e) * 2], row = stab[(srow * Ss + e) * 2 + 1];
    if (i < 0) continue;
    s += dout[(b * N + i) * out_w + col0 + c] * we[(b * we_rows + row) * we_w + c];
  }
  dhx[(b * hx_rows + srow) * hx_w + c] += s;
}

// ---- head: FINAL, SLOGDET, ORBITALS ----

// One thread per walker.  With c = cot (0 for a walker whose sign is 0 or whose log|psi| is not finite) and the CI weights
// p_k = c_k s_k exp(L_k - log|sum|): dL[b][k] = c p_k; per-walker partials pw[b][K + 2] of d/dc_k (c s_k exp(L_k) / sum)
// and of the two cusp alphas; the Jastrow output receives c.
template <typename real>
__global__ void __launch_bounds__(256) k_final_bwd(const real* __restrict__ r, const double* __restrict__ logdet,
                                                   const int32_t* __restrict__ sign_k, const real* __restrict__ cc,
                                                   const real* __restrict__ alphas, int cusp_kind, double same_scale, double anti_scale,
                                                   double eps, const real* __restrict__ logpsi, const int32_t* __restrict__ sign,
                                                   const real* __restrict__ cot, real* __restrict__ djas, int jas_ld,
                                                   double* __restrict__ dL, double* __restrict__ pw, int B, int N, int n_up, int K) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double c = cot ? (double)cot[b] : 1.0;
  const double lp = (double)logpsi[b];
  if (sign[b] == 0 || !(lp - lp == 0)) c = 0;
  double* p = pw + (long)b * (K + 2);
  if (djas) djas[(long)b * jas_ld] += (real)c;
  if (c == 0) {
    for (int k = 0; k < K; ++k) { dL[(long)b * K + k] = 0; p[k] = 0; }
    p[K] = p[K + 1] = 0;
    return;
  }
  double shift = -INFINITY;
  for (int k = 0; k < K; ++k) shift = fmax(shift, logdet[(long)b * K + k]);
  if (!(shift - shift == 0)) shift = 0;
  double psi = 0;
  for (int k = 0; k < K; ++k)
    psi += (cc ? (double)cc[k] : 1.0) * sign_k[(long)b * K + k] * exp(logdet[(long)b * K + k] - shift);
  for (int k = 0; k < K; ++k) {
    const double e = sign_k[(long)b * K + k] * exp(logdet[(long)b * K + k] - shift) / psi;
    p[k] = c * e;
    dL[(long)b * K + k] = c * (cc ? (double)cc[k] : 1.0) * e;
  }
  double d_same = 0, d_anti = 0;
  if (cusp_kind) {
    const double a_same = (double)alphas[0], a_anti = (double)alphas[1];
    const real* rb = r + (long)b * N * 3;
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) {
        double d2 = eps;
        for (int x = 0; x < 3; ++x) { const double d = (double)rb[i * 3 + x] - (double)rb[j * 3 + x]; d2 += d * d; }
        const double rho = sqrt(d2);
        const bool same = (i < n_up) == (j < n_up);
        const double sc = same ? same_scale : anti_scale, al = same ? a_same : a_anti;
        double g;
        if (cusp_kind == 1) { const double q = al * (1 + al * rho); g = sc * (1 + 2 * al * rho) / (q * q); }
        else g = -sc * al * (al + 2 * rho) / ((al + rho) * (al + rho));
        if (same) d_same += g; else d_anti += g;
      }
  }
  p[K] = c * d_same;
  p[K + 1] = c * d_anti;
}

// dA_k = dL_k A_k^-T for one (walker, determinant) per workgroup: Gauss-Jordan with partial pivoting on [A | I] in LDS,
// double, N <= GRAD_GJ_NMAX = 64.  Matrices with dL_k = 0 (no weight, or a singular A_k: s_k = 0) keep a zero adjoint.

template <typename real>
__global__ void __launch_bounds__(64) k_slogdet_bwd(const real* __restrict__ orb, int orb_w, const double* __restrict__ dL,
                                                    real* __restrict__ dorb, int N) {
  HIP_DYNAMIC_SHARED(char, smem_raw)                 // M[N][2 N], f[N]: 66 KB at N = 64 (slogdet_bwd_set_lds_limit)
  __shared__ int piv;
  const long mat = blockIdx.x;
  const int t = threadIdx.x, W = 2 * N;
  double* M = reinterpret_cast<double*>(smem_raw);
  double* f = M + N * W;
  const double g = dL[mat];
  if (g == 0) return;
  const real* A = orb + mat * orb_w;
  for (int e = t; e < N * W; e += 64) {
    const int i = e / W, j = e - i * W;
    M[e] = j < N ? (double)A[i * N + j] : (j - N == i ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int c = 0; c < N; ++c) {
    if (t == 0) {
      int p = c;
      double best = fabs(M[c * W + c]);
      for (int q = c + 1; q < N; ++q) if (fabs(M[q * W + c]) > best) { best = fabs(M[q * W + c]); p = q; }
      piv = p;
    }
    __syncthreads();
    const int p = piv;
    if (p != c)
      for (int j = t; j < W; j += 64) { const double x = M[c * W + j]; M[c * W + j] = M[p * W + j]; M[p * W + j] = x; }
    __syncthreads();
    const double inv_pv = 1.0 / M[c * W + c];
    __syncthreads();
    for (int j = t; j < W; j += 64) M[c * W + j] *= inv_pv;
    for (int q = t; q < N; q += 64) f[q] = M[q * W + c];
    __syncthreads();
    for (int e = t; e < N * W; e += 64) {
      const int q = e / W, j = e - q * W;
      if (q != c) M[e] -= f[q] * M[c * W + j];
    }
    __syncthreads();
  }
  real* dA = dorb + mat * orb_w;
  for (int e = t; e < N * N; e += 64) {
    const int i = e / N, mu = e - i * N;
    dA[e] = (real)(g * M[mu * W + N + i]);         // (A^-T)[i][mu] = (A^-1)[mu][i]
  }
}

// ORBITALS: A_k[i][mu] = env_i[k N + mu] bf[i][k N + mu], env_i[o] = sum_a pi[o][a] exp(-|zeta[o][a]| rho_ia) with the tables of
// electron i's spin.  One thread per (walker, spin, orbital column o): the backflow adjoint of every electron of that spin, and
// the per-walker partials pw[b][t][o][a] of the four tables t = pi_up, pi_down, zeta_up, zeta_down.
template <typename real>
__global__ void __launch_bounds__(256) k_orbitals_bwd(const real* __restrict__ r, const real* __restrict__ R, const real* __restrict__ bf,
                                                      int bf_w, real* __restrict__ dbf, const real* __restrict__ dorb, int orb_w,
                                                      const real* __restrict__ pi_up, const real* __restrict__ pi_dn,
                                                      const real* __restrict__ ze_up, const real* __restrict__ ze_dn,
                                                      double* __restrict__ pw, int B, int N, int n_up, int n_env, int n_nuc, int K,
                                                      double eps) {
  const int KN = K * N, L = n_nuc * n_env;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * 2 * KN) return;
  const int o = (int)(idx % KN);
  const int sp = (int)((idx / KN) % 2);
  const long b = idx / (2L * KN);
  const int k = o / N, mu = o - k * N;
  const int lo = sp ? n_up : 0, hi = sp ? N : n_up;
  const real* pi = (sp ? pi_dn : pi_up) + (long)o * L;
  const real* ze = (sp ? ze_dn : ze_up) + (long)o * L;
  double* p_pi = pw ? pw + ((long)b * 4 + sp) * KN * L + (long)o * L : nullptr;
  double* p_ze = pw ? pw + ((long)b * 4 + 2 + sp) * KN * L + (long)o * L : nullptr;
  const real* rb = r + (long)b * N * 3;
  for (int a = 0; pw && a < L; ++a) {      // table partials (none without pw)
    const int nuc = a / n_env;
    const double z = (double)ze[a], az = fabs(z), sz = (double)((z > 0) - (z < 0));
    double s_pi = 0, s_ze = 0;
    for (int i = lo; i < hi; ++i) {
      double d2 = eps;
      for (int x = 0; x < 3; ++x) { const double d = (double)rb[i * 3 + x] - (double)R[nuc * 3 + x]; d2 += d * d; }
      const double rho = sqrt(d2), ex = exp(-az * rho);
      const double t = (double)dorb[(b * K + k) * orb_w + i * N + mu] * (double)bf[(b * N + i) * bf_w + o];
      s_pi += t * ex;
      s_ze -= t * (double)pi[a] * ex * rho * sz;
    }
    p_pi[a] = s_pi;
    p_ze[a] = s_ze;
  }
  for (int i = lo; i < hi; ++i) {
    double env = 0;
    for (int a = 0; a < L; ++a) {
      const int nuc = a / n_env;
      double d2 = eps;
      for (int x = 0; x < 3; ++x) { const double d = (double)rb[i * 3 + x] - (double)R[nuc * 3 + x]; d2 += d * d; }
      env += (double)pi[a] * exp(-fabs((double)ze[a]) * sqrt(d2));
    }
    dbf[(b * N + i) * bf_w + o] += (real)((double)dorb[(b * K + k) * orb_w + i * N + mu] * env);
  }
}

// ---- launchers ----

static inline unsigned grad_grid(long n) { return (unsigned)((n + 255) / 256); }

template <typename real>
void launch_linear_bwd(hipStream_t st, const LinBwdArgs<real>& a) {
  const long M = (long)a.B * a.nrows, nz = M * a.ldw;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dz<real>), dim3(grad_grid(nz)), dim3(256), 0, st, a.Z, a.dZ, a.dY, a.ld_dst, a.rpw_dst,
                     a.r0_dst, a.col0_dst, a.dres, a.ld_res, a.rpw_res, a.r0_res, a.dres ? a.res_scale : (real)1, a.act, a.nrows,
                     a.nout, a.ldw, nz);
  const int Nt = (a.ldw + 15) / 16;
  // weight gradient: split-K over the rows (about GRAD_DW_WAVES waves per launch), S partial tiles per 16 x 16 block, then
  // their fixed-order sum; the bias is the block of a constant-one input row
  auto dw = [&](const real* X, int ld, int rpw, int r0, int bcast, int K, double* g) {
    const int kt = (K + 15) / 16;
    const long S0 = grad_dw_splits(kt, Nt, M);
    const long m_per = ((M + S0 - 1) / S0 + 3) / 4 * 4;
    const long S = (M + m_per - 1) / m_per;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dw<real>), dim3((unsigned)kt, (unsigned)Nt, (unsigned)S), dim3(64), 0, st, X, ld, rpw, r0,
                       bcast, K, (const real*)a.dZ, a.ldw, a.nrows, M, m_per, a.part, a.wt);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dw_reduce), dim3(grad_grid((long)K * a.nout)), dim3(256), 0, st, (const double*)a.part,
                       (int)S, kt * 16, Nt * 16, K, a.nout, a.ldw, g);
  };
  if (a.dbias) dw(nullptr, 0, 1, 0, 0, 1, a.dbias);
  for (int p = 0; p < a.n_pieces; ++p) {
    const LinBwdPiece<real>& q = a.piece[p];
    const int kt = (q.K + 15) / 16;
    if (a.dW) dw(q.X, q.ld, q.rpw, q.r0, q.bcast, q.K, a.dW + (long)q.w_row * a.ldw);
    if (!q.dX) continue;
    // input adjoint; a broadcast piece first sums the segment's rows of dZ per walker
    if (q.bcast) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dz_rowsum<real>), dim3(grad_grid((long)a.B * a.ldw)), dim3(256), 0, st,
                         (const real*)a.dZ, a.dZs, a.nrows, a.ldw, (long)a.B * a.ldw);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dx<real>), dim3((unsigned)((a.B + 63) / 64), (unsigned)kt), dim3(256), 0, st,
                         (const real*)a.dZs, 1, (long)a.B, a.W, a.ldw, q.w_row, q.K, q.dX, q.ld, q.rpw, q.r0);
    } else {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_dx<real>), dim3((unsigned)((M + 63) / 64), (unsigned)kt), dim3(256), 0, st,
                         (const real*)a.dZ, a.nrows, M, a.W, a.ldw, q.w_row, q.K, q.dX, q.ld, q.rpw, q.r0);
    }
  }
}

template <typename real>
void launch_colsum(hipStream_t st, const real* in, long count, long stride, int m, double* out, const double* wt) {
  if (m > 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_colsum<real>), dim3((unsigned)m), dim3(256), 0, st, in, count, stride, out, wt);
}
void launch_colsum_f64(hipStream_t st, const double* in, long count, long stride, int m, double* out, const double* wt) {
  if (m > 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_colsum<double>), dim3((unsigned)m), dim3(256), 0, st, in, count, stride, out, wt);
}

template <typename real>
void launch_spin_mean_bwd(hipStream_t st, real* dx, const real* dm, int B, int N, int n_up, int width) {
  const long n = (long)B * N * width;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spin_mean_bwd<real>), dim3(grad_grid(n)), dim3(256), 0, st, dx, dm, N, n_up, width, n);
}
template <typename real>
void launch_row_sum_bwd(hipStream_t st, real* dx, const real* ds, int B, int rows, int width) {
  const long n = (long)B * rows * width;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_row_sum_bwd<real>), dim3(grad_grid(n)), dim3(256), 0, st, dx, ds, rows, width, n);
}
template <typename real>
void launch_edge_rows_bwd(hipStream_t st, real* dwe, int we_rows, int we_w, const real* hx, int hx_rows, int hx_w, const real* dout,
                          int out_w, int col0, const int32_t* rtab, int Sr, int W, int B, int N, double scale) {
  const long n = (long)B * we_rows * W;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_edge_rows_bwd<real>), dim3(grad_grid(n)), dim3(256), 0, st, dwe, we_rows, we_w, hx, hx_rows, hx_w,
                     dout, out_w, col0, rtab, Sr, W, N, (real)scale, n);
}
template <typename real>
void launch_conv_send_bwd(hipStream_t st, real* dhx, int hx_rows, int hx_w, const real* we, int we_rows, int we_w, const real* dout,
                          int out_w, int col0, const int32_t* stab, int Ss, int W, int B, int N) {
  const long n = (long)B * hx_rows * W;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_conv_send_bwd<real>), dim3(grad_grid(n)), dim3(256), 0, st, dhx, hx_rows, hx_w, we, we_rows, we_w,
                     dout, out_w, col0, stab, Ss, W, N, n);
}
template <typename real>
void launch_final_bwd(hipStream_t st, const FinalBwdArgs<real>& a) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_final_bwd<real>), dim3(grad_grid(a.B)), dim3(256), 0, st, a.r, a.logdet, a.sign_k, a.cc, a.alphas,
                     a.cusp_kind, a.same_scale, a.anti_scale, a.eps, a.logpsi, a.sign, a.cot, a.djas, a.jas_ld, a.dL, a.pw, a.B, a.N,
                     a.n_up, a.K);
}
template <typename real>
void launch_slogdet_bwd(hipStream_t st, const real* orb, int orb_w, const double* dL, real* dorb, int B, int K, int N) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_slogdet_bwd<real>), dim3((unsigned)((long)B * K)), dim3(64), sizeof(double) * ((size_t)2 * N * N + N), st, orb, orb_w, dL, dorb, N);
}
// (called when a context of more than 44 electrons is created: the launch itself may be part of a captured graph)
template <typename real> int slogdet_bwd_set_lds_limit() {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_slogdet_bwd<real>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(double) * (2 * GRAD_GJ_NMAX * GRAD_GJ_NMAX + GRAD_GJ_NMAX)));
}
template int slogdet_bwd_set_lds_limit<float>();
template int slogdet_bwd_set_lds_limit<double>();
template <typename real>
void launch_orbitals_bwd(hipStream_t st, const real* r, const real* R, const real* bf, int bf_w, real* dbf, const real* dorb, int orb_w,
                         const real* pi_up, const real* pi_dn, const real* ze_up, const real* ze_dn, double* pw, int B, int N, int n_up,
                         int n_env, int n_nuc, int K, double eps) {
  const long n = (long)B * 2 * K * N;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_orbitals_bwd<real>), dim3(grad_grid(n)), dim3(256), 0, st, r, R, bf, bf_w, dbf, dorb, orb_w, pi_up,
                     pi_dn, ze_up, ze_dn, pw, B, N, n_up, n_env, n_nuc, K, eps);
}

#define DQMC_GRAD_INST(real)                                                                                                        \
  template void launch_linear_bwd<real>(hipStream_t, const LinBwdArgs<real>&);                                                    \
  template void launch_colsum<real>(hipStream_t, const real*, long, long, int, double*, const double*);                           \
  template void launch_spin_mean_bwd<real>(hipStream_t, real*, const real*, int, int, int, int);                                  \
  template void launch_row_sum_bwd<real>(hipStream_t, real*, const real*, int, int, int);                                         \
  template void launch_edge_rows_bwd<real>(hipStream_t, real*, int, int, const real*, int, int, const real*, int, int,            \
                                           const int32_t*, int, int, int, int, double);                                           \
  template void launch_conv_send_bwd<real>(hipStream_t, real*, int, int, const real*, int, int, const real*, int, int,            \
                                           const int32_t*, int, int, int, int);                                                   \
  template void launch_final_bwd<real>(hipStream_t, const FinalBwdArgs<real>&);                                                   \
  template void launch_slogdet_bwd<real>(hipStream_t, const real*, int, const double*, real*, int, int, int);                     \
  template void launch_orbitals_bwd<real>(hipStream_t, const real*, const real*, const real*, int, real*, const real*, int,       \
                                          const real*, const real*, const real*, const real*, double*, int, int, int, int, int,   \
                                          int, double);
DQMC_GRAD_INST(float)
DQMC_GRAD_INST(double)
#undef DQMC_GRAD_INST

}  // namespace dqmc
