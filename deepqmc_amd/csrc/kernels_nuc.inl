// kernels_nuc.inl -- included by kernel_attention.hip (inside namespace dqmc): the nuclear-token stream of the TransPsiformer
// on the device (engine_nuc.inl: nuc_fold, nuc_fold_vjp; the host form is deepqmc_amd/nuclear_stream.py).
//
// Always float64, in float32 contexts too: theta is float64, the host fold is float64, and the whole stream is a few MFLOP.
// Rows are the n_nuc tokens (or the n_nuc^2 edges of the nuclei embedding), widths the embedding width and the 32 of the edge
// MLP: small dedicated kernels, one thread per output element, every sum in ascending index order, no atomics.  Gradients
// of parameters are ADDED into the caller's vector (the electron stream's gradient of the shared leaves is already there).
// Activation codes as DQMC_OP_LINEAR: 0 none, 1 tanh, 2 silu.

constexpr int NUC_BLOCK = 128;
static inline unsigned nuc_grid(long n) { return (unsigned)((n + NUC_BLOCK - 1) / NUC_BLOCK); }

__device__ inline double nuc_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ inline double nuc_act(double z, int act) {
  if (act == 1) return tanh(z);
  if (act == 2) return z * nuc_sigmoid(z);
  return z;
}
__device__ inline double nuc_dact(double z, int act) {
  if (act == 1) { const double t = tanh(z); return 1.0 - t * t; }
  if (act == 2) { const double s = nuc_sigmoid(z); return s * (1.0 + z * (1.0 - s)); }
  return 1.0;
}

// F[(s n + r)][4 + n]: features of d = R[r] - R[s] (|d| and d, log-rescaled under the safe norm) and the one-hot atom type of
// the sender s (nuclear_stream.nuclei_embedding)
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_edge_feat(const double* __restrict__ R, const int32_t* __restrict__ types, double eps,
                                                             double* __restrict__ F, int n) {
  const int e = blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= n * n) return;
  const int s = e / n, r = e - s * n, w = 4 + n;
  const double dx = R[3 * r] - R[3 * s], dy = R[3 * r + 1] - R[3 * s + 1], dz = R[3 * r + 2] - R[3 * s + 2];
  const double rho = sqrt(eps + (dx * dx + dy * dy + dz * dz));
  const double sc = log1p(rho) / rho;
  double* f = F + (long)e * w;
  f[0] = rho * sc; f[1] = dx * sc; f[2] = dy * sc; f[3] = dz * sc;
  for (int c = 0; c < n; ++c) f[4 + c] = c == types[s] ? 1.0 : 0.0;
}

// Z = X W + b (kept when Z != Y: the backward needs the pre-activation), Y = act(Z) (+ res).  X [rows][n_in], W [n_in][n_out]
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_linear(const double* __restrict__ X, const double* __restrict__ W,
                                                          const double* __restrict__ b, double* __restrict__ Z, double* __restrict__ Y,
                                                          const double* __restrict__ res, int rows, int n_in, int n_out, int act) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= (long)rows * n_out) return;
  const int r = (int)(e / n_out), o = (int)(e - (long)r * n_out);
  double z = 0.0;
  for (int i = 0; i < n_in; ++i) z += X[(long)r * n_in + i] * W[(long)i * n_out + o];
  if (b) z += b[o];
  if (Z != Y) Z[e] = z;
  double y = nuc_act(z, act);
  if (res) y += res[e];
  Y[e] = y;
}
// dZ = dY act'(Z) (act != 0: Z and dZ are buffers of their own)
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_dz(const double* __restrict__ dY, const double* __restrict__ Z, double* __restrict__ dZ,
                                                      long n, int act) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e < n) dZ[e] = dY[e] * nuc_dact(Z[e], act);
}
// dX[r][i] += sum_o dZ[r][o] W[i][o]
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_dx(const double* __restrict__ dZ, const double* __restrict__ W, double* __restrict__ dX,
                                                      int rows, int n_in, int n_out) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= (long)rows * n_in) return;
  const int r = (int)(e / n_in), i = (int)(e - (long)r * n_in);
  double a = 0.0;
  for (int o = 0; o < n_out; ++o) a += dZ[(long)r * n_out + o] * W[(long)i * n_out + o];
  dX[e] += a;
}
// gW[i][o] += sum_r X[r][i] dZ[r][o]; elements n_in * n_out .. + n_out - 1 of the launch: gb[o] += sum_r dZ[r][o]
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_dw(const double* __restrict__ X, const double* __restrict__ dZ, double* __restrict__ gW,
                                                      double* __restrict__ gb, int rows, int n_in, int n_out) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  const long nw = (long)n_in * n_out;
  if (e < nw) {
    const int i = (int)(e / n_out), o = (int)(e - (long)i * n_out);
    double a = 0.0;
    for (int r = 0; r < rows; ++r) a += X[(long)r * n_in + i] * dZ[(long)r * n_out + o];
    gW[e] += a;
  } else if (gb && e < nw + n_out) {
    const int o = (int)(e - nw);
    double a = 0.0;
    for (int r = 0; r < rows; ++r) a += dZ[(long)r * n_out + o];
    gb[o] += a;
  }
}
// out[r][c] = sum_s in[s n + r][c]
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_sender_sum(const double* __restrict__ in, double* __restrict__ out, int n, int w) {
  const int e = blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= n * w) return;
  double a = 0.0;
  for (int s = 0; s < n; ++s) a += in[(long)s * n * w + e];
  out[e] = a;
}
// din[s n + r][c] += dout[r][c]
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_sender_sum_bwd(const double* __restrict__ dout, double* __restrict__ din, int n, int w) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e < (long)n * n * w) din[e] += dout[e % ((long)n * w)];
}
// a += b
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_add(double* __restrict__ a, const double* __restrict__ b, long n) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e < n) a[e] += b[e];
}

// Softmax attention among the n tokens; one workgroup per head, thread t owns query row t: P[h][t][:] (kept for the backward)
// and o[t][h hd ..].  q, k, v, o: [n][H hd].
__global__ void __launch_bounds__(64) k_nuc_attention(const double* __restrict__ q, const double* __restrict__ k, const double* __restrict__ v,
                                                      double* __restrict__ P, double* __restrict__ o, int n, int H, int hd) {
  const int h = blockIdx.x, t = threadIdx.x, D = H * hd, c0 = h * hd;
  if (t >= n) return;
  double* Pr = P + ((long)h * n + t) * n;
  const double sc = 1.0 / sqrt((double)hd);
  double mx = 0.0;
  for (int T = 0; T < n; ++T) {
    double s = 0.0;
    for (int d = 0; d < hd; ++d) s += q[(long)t * D + c0 + d] * k[(long)T * D + c0 + d];
    s *= sc;
    Pr[T] = s;
    mx = (T == 0 || s > mx) ? s : mx;
  }
  double sum = 0.0;
  for (int T = 0; T < n; ++T) { const double ev = exp(Pr[T] - mx); Pr[T] = ev; sum += ev; }
  const double inv = 1.0 / sum;
  for (int T = 0; T < n; ++T) Pr[T] *= inv;
  for (int d = 0; d < hd; ++d) {
    double a = 0.0;
    for (int T = 0; T < n; ++T) a += Pr[T] * v[(long)T * D + c0 + d];
    o[(long)t * D + c0 + d] = a;
  }
}
// first half of its backward: thread t forms dS[h][t][:] = P (dP - sum P dP), dP = do v^T, and adds dq[t] = s dS k
__global__ void __launch_bounds__(64) k_nuc_attention_bwd_q(const double* __restrict__ k, const double* __restrict__ v,
                                                            const double* __restrict__ P, const double* __restrict__ dO,
                                                            double* __restrict__ dS, double* __restrict__ dq, int n, int H, int hd) {
  const int h = blockIdx.x, t = threadIdx.x, D = H * hd, c0 = h * hd;
  if (t >= n) return;
  const double* Pr = P + ((long)h * n + t) * n;
  double* dSr = dS + ((long)h * n + t) * n;
  const double sc = 1.0 / sqrt((double)hd);
  double m = 0.0;
  for (int T = 0; T < n; ++T) {
    double p = 0.0;
    for (int d = 0; d < hd; ++d) p += dO[(long)t * D + c0 + d] * v[(long)T * D + c0 + d];
    dSr[T] = p;
    m += Pr[T] * p;
  }
  for (int T = 0; T < n; ++T) dSr[T] = Pr[T] * (dSr[T] - m);
  for (int d = 0; d < hd; ++d) {
    double a = 0.0;
    for (int T = 0; T < n; ++T) a += dSr[T] * k[(long)T * D + c0 + d];
    dq[(long)t * D + c0 + d] += sc * a;
  }
}
// second half (a launch of its own: it reads every row of dS): thread T adds dk[T] = s dS^T q and dv[T] = P^T do
__global__ void __launch_bounds__(64) k_nuc_attention_bwd_kv(const double* __restrict__ q, const double* __restrict__ P,
                                                             const double* __restrict__ dS, const double* __restrict__ dO,
                                                             double* __restrict__ dk, double* __restrict__ dv, int n, int H, int hd) {
  const int h = blockIdx.x, T = threadIdx.x, D = H * hd, c0 = h * hd;
  if (T >= n) return;
  const double sc = 1.0 / sqrt((double)hd);
  for (int d = 0; d < hd; ++d) {
    double ak = 0.0, av = 0.0;
    for (int t = 0; t < n; ++t) {
      ak += dS[((long)h * n + t) * n + T] * q[(long)t * D + c0 + d];
      av += P[((long)h * n + t) * n + T] * dO[(long)t * D + c0 + d];
    }
    dk[(long)T * D + c0 + d] += sc * ak;
    dv[(long)T * D + c0 + d] += av;
  }
}

// hk.LayerNorm(-1, no scale, no offset, eps 1e-5) per row; rstd[r] is kept for the backward
__global__ void __launch_bounds__(64) k_nuc_layernorm(const double* __restrict__ h, double* __restrict__ ln, double* __restrict__ rstd, int n,
                                                      int D) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n) return;
  double mu = 0.0;
  for (int c = 0; c < D; ++c) mu += h[(long)r * D + c];
  mu /= D;
  double var = 0.0;
  for (int c = 0; c < D; ++c) { const double d = h[(long)r * D + c] - mu; var += d * d; }
  var /= D;
  const double rs = 1.0 / sqrt(var + 1e-5);
  for (int c = 0; c < D; ++c) ln[(long)r * D + c] = (h[(long)r * D + c] - mu) * rs;
  rstd[r] = rs;
}
// dh += rstd (dln - mean(dln) - ln mean(dln ln))
__global__ void __launch_bounds__(64) k_nuc_layernorm_bwd(const double* __restrict__ ln, const double* __restrict__ rstd,
                                                          const double* __restrict__ dln, double* __restrict__ dh, int n, int D) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n) return;
  double a = 0.0, b = 0.0;
  for (int c = 0; c < D; ++c) { a += dln[(long)r * D + c]; b += dln[(long)r * D + c] * ln[(long)r * D + c]; }
  a /= D; b /= D;
  for (int c = 0; c < D; ++c) dh[(long)r * D + c] += rstd[r] * (dln[(long)r * D + c] - a - ln[(long)r * D + c] * b);
}
// zeta = sigmoid(zw) zv + bias
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_glu(const double* __restrict__ zw, const double* __restrict__ zv,
                                                       const double* __restrict__ bias, double* __restrict__ zeta, long n) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e < n) zeta[e] = nuc_sigmoid(zw[e]) * zv[e] + bias[e];
}
// dzw = dzeta zv sig (1 - sig), dzv = dzeta sig, gbias += dzeta
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_glu_bwd(const double* __restrict__ zw, const double* __restrict__ zv,
                                                           const double* __restrict__ dzeta, double* __restrict__ dzw, double* __restrict__ dzv,
                                                           double* __restrict__ gbias, long n) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= n) return;
  const double s = nuc_sigmoid(zw[e]), g = dzeta[e];
  dzw[e] = g * zv[e] * s * (1.0 - s);
  dzv[e] = g * s;
  gbias[e] += g;
}
// every weight entry that is a copy of derived element e: w (the context's precision) and w64 (float32 contexts, or nullptr)
template <typename real>
__global__ void __launch_bounds__(NUC_BLOCK) k_nuc_scatter(const double* __restrict__ derived, const int32_t* __restrict__ row,
                                                           const int32_t* __restrict__ col, real* __restrict__ w, double* __restrict__ w64,
                                                           long n) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (e >= n) return;
  const double v = derived[e];
  for (int32_t k = row[e]; k < row[e + 1]; ++k) {
    w[col[k]] = (real)v;
    if (w64) w64[col[k]] = v;
  }
}

void launch_nuc_edge_feat(hipStream_t st, const double* R, const int32_t* types, double eps, double* F, int n) {
  hipLaunchKernelGGL(k_nuc_edge_feat, dim3(nuc_grid((long)n * n)), dim3(NUC_BLOCK), 0, st, R, types, eps, F, n);
}
void launch_nuc_linear(hipStream_t st, const double* X, const double* W, const double* b, double* Z, double* Y, const double* res, int rows,
                       int n_in, int n_out, int act) {
  hipLaunchKernelGGL(k_nuc_linear, dim3(nuc_grid((long)rows * n_out)), dim3(NUC_BLOCK), 0, st, X, W, b, Z, Y, res, rows, n_in, n_out, act);
}
void launch_nuc_linear_bwd(hipStream_t st, const double* X, const double* W, const double* Z, const double* dY, double* dZ, double* dX,
                           double* gW, double* gb, int rows, int n_in, int n_out, int act) {
  const double* dz = dY;
  if (act != 0) {
    hipLaunchKernelGGL(k_nuc_dz, dim3(nuc_grid((long)rows * n_out)), dim3(NUC_BLOCK), 0, st, dY, Z, dZ, (long)rows * n_out, act);
    dz = dZ;
  }
  hipLaunchKernelGGL(k_nuc_dw, dim3(nuc_grid((long)n_in * n_out + n_out)), dim3(NUC_BLOCK), 0, st, X, dz, gW, gb, rows, n_in, n_out);
  if (dX) hipLaunchKernelGGL(k_nuc_dx, dim3(nuc_grid((long)rows * n_in)), dim3(NUC_BLOCK), 0, st, dz, W, dX, rows, n_in, n_out);
}
void launch_nuc_sender_sum(hipStream_t st, const double* in, double* out, int n, int w) {
  hipLaunchKernelGGL(k_nuc_sender_sum, dim3(nuc_grid((long)n * w)), dim3(NUC_BLOCK), 0, st, in, out, n, w);
}
void launch_nuc_sender_sum_bwd(hipStream_t st, const double* dout, double* din, int n, int w) {
  hipLaunchKernelGGL(k_nuc_sender_sum_bwd, dim3(nuc_grid((long)n * n * w)), dim3(NUC_BLOCK), 0, st, dout, din, n, w);
}
void launch_nuc_add(hipStream_t st, double* a, const double* b, long n) {
  hipLaunchKernelGGL(k_nuc_add, dim3(nuc_grid(n)), dim3(NUC_BLOCK), 0, st, a, b, n);
}
void launch_nuc_attention(hipStream_t st, const double* q, const double* k, const double* v, double* P, double* o, int n, int H, int hd) {
  hipLaunchKernelGGL(k_nuc_attention, dim3((unsigned)H), dim3(64), 0, st, q, k, v, P, o, n, H, hd);
}
void launch_nuc_attention_bwd(hipStream_t st, const double* q, const double* k, const double* v, const double* P, const double* dO, double* dS,
                              double* dq, double* dk, double* dv, int n, int H, int hd) {
  hipLaunchKernelGGL(k_nuc_attention_bwd_q, dim3((unsigned)H), dim3(64), 0, st, k, v, P, dO, dS, dq, n, H, hd);
  hipLaunchKernelGGL(k_nuc_attention_bwd_kv, dim3((unsigned)H), dim3(64), 0, st, q, P, dS, dO, dk, dv, n, H, hd);
}
void launch_nuc_layernorm(hipStream_t st, const double* h, double* ln, double* rstd, int n, int D) {
  hipLaunchKernelGGL(k_nuc_layernorm, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, h, ln, rstd, n, D);
}
void launch_nuc_layernorm_bwd(hipStream_t st, const double* ln, const double* rstd, const double* dln, double* dh, int n, int D) {
  hipLaunchKernelGGL(k_nuc_layernorm_bwd, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, ln, rstd, dln, dh, n, D);
}
void launch_nuc_glu(hipStream_t st, const double* zw, const double* zv, const double* bias, double* zeta, long n) {
  hipLaunchKernelGGL(k_nuc_glu, dim3(nuc_grid(n)), dim3(NUC_BLOCK), 0, st, zw, zv, bias, zeta, n);
}
void launch_nuc_glu_bwd(hipStream_t st, const double* zw, const double* zv, const double* dzeta, double* dzw, double* dzv, double* gbias,
                        long n) {
  hipLaunchKernelGGL(k_nuc_glu_bwd, dim3(nuc_grid(n)), dim3(NUC_BLOCK), 0, st, zw, zv, dzeta, dzw, dzv, gbias, n);
}
template <typename real>
void launch_nuc_scatter(hipStream_t st, const double* derived, const int32_t* row, const int32_t* col, real* w, double* w64, long n) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nuc_scatter<real>), dim3(nuc_grid(n)), dim3(NUC_BLOCK), 0, st, derived, row, col, w, w64, n);
}
template void launch_nuc_scatter<float>(hipStream_t, const double*, const int32_t*, const int32_t*, float*, double*, long);
template void launch_nuc_scatter<double>(hipStream_t, const double*, const int32_t*, const int32_t*, double*, double*, long);
