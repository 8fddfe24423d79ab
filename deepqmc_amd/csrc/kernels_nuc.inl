// kernels_nuc.inl -- included by kernel_attention.hip (inside namespace dqmc): the nuclear-token stream of the TransPsiformer
// on the device (engine_nuc.inl: nuc_fold, nuc_fold_vjp; the host form is deepqmc_amd/nuclear_stream.py).
//
// Always float64, in float32 contexts too: theta is float64, the host fold is float64, and the whole stream is a few MFLOP.
// Rows are the n_nuc tokens (or the n_nuc^2 edges of the nuclei embedding), widths the embedding width and the 32 of the edge
// MLP: small dedicated kernels, one thread per output element, every sum in ascending index order, no atomics.  Gradients
// of parameters are ADDED into the caller's vector (the electron stream's gradient of the shared leaves is already there).
// Activation codes as DQMC_OP_LINEAR: 0 none, 1 tanh, 2 silu.
// The k_nucb_* kernels further down are the backward once more, batched over the walkers of a chunk of the coordinate reverse
// pass (option "nuclear_coords"): adjoints only, rows B n or B n^2, the linear layers on the float64 MFMA.

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

// ---- the stream's backward batched over walkers: adjoints only, down to R (engine_nuc.inl: nuc_fold_coords) ----
// Every walker b has an adjoint arena of its own, G + b * A, laid out like nuc_adj (A = the arena's length); the activations
// (Z, Y, P, ln, rstd) and the weights are the shared ones of the last fold.  Offsets into the arena are passed as pointers
// into walker 0's arena.  One thread (or one wave tile) owns every element it adds into, sums run in ascending index order:
// no atomics, two identical calls give identical bits.

// G[b][e] += the sum of walker b's partials src[b * stride + (col - w0)] over the copies col of derived element e that lie in
// the weight range [w0, w0 + len), in the order of the CSR table; e in [e_lo, e_hi)
template <typename T>
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_gather(const T* __restrict__ src, long stride, long w0, long len,
                                                           const int32_t* __restrict__ row, const int32_t* __restrict__ col, long e_lo,
                                                           long e_hi, double* __restrict__ G, long A, long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long ne = e_hi - e_lo, b = idx / ne, e = e_lo + (idx - b * ne);
  double s = 0.0;
  for (int32_t k = row[e]; k < row[e + 1]; ++k) {
    const long c = (long)col[k] - w0;
    if (c >= 0 && c < len) s += (double)src[b * stride + c];
  }
  G[b * A + e] += s;
}
// a[b][e] += c[b][e], e < n
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_add(double* __restrict__ a, const double* __restrict__ c, long n, long A, long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n, e = idx - b * n;
  a[b * A + e] += c[b * A + e];
}
// dzw = dzeta zv sig (1 - sig), dzv = dzeta sig (no bias gradient)
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_glu_bwd(const double* __restrict__ zw, const double* __restrict__ zv,
                                                            const double* __restrict__ dzeta, double* __restrict__ dzw,
                                                            double* __restrict__ dzv, long n, long A, long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n, e = idx - b * n;
  const double s = nuc_sigmoid(zw[e]), g = dzeta[b * A + e];
  dzw[b * A + e] = g * zv[e] * s * (1.0 - s);
  dzv[b * A + e] = g * s;
}
// dh += rstd (dln - mean(dln) - ln mean(dln ln)); one thread per (walker, row)
__global__ void __launch_bounds__(64) k_nucb_layernorm_bwd(const double* __restrict__ ln, const double* __restrict__ rstd,
                                                           const double* __restrict__ dln, double* __restrict__ dh, int n, int D, long A,
                                                           long total) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n;
  const int r = (int)(idx - b * n);
  const double* g = dln + b * A + (long)r * D;
  const double* l = ln + (long)r * D;
  double a = 0.0, c = 0.0;
  for (int k = 0; k < D; ++k) { a += g[k]; c += g[k] * l[k]; }
  a /= D; c /= D;
  double* o = dh + b * A + (long)r * D;
  for (int k = 0; k < D; ++k) o[k] += rstd[r] * (g[k] - a - l[k] * c);
}
// din[b][s n + r][c] += dout[b][r][c]
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_sender_sum_bwd(const double* __restrict__ dout, double* __restrict__ din, int n, int w,
                                                                   long A, long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long per = (long)n * n * w, b = idx / per, e = idx - b * per;
  din[b * A + e] += dout[b * A + e % ((long)n * w)];
}
// Token attention backward, one workgroup per (walker, head), thread t owns query row t and then key row t.  P is shared,
// dO per walker: dS[t][:] = P (dP - sum P dP) with dP = dO v^T goes to the LDS ([n][n + 1] doubles), dq[t] += s dS k; after
// the barrier dk[T] += s dS^T q, dv[T] += P^T dO.
__global__ void __launch_bounds__(64) k_nucb_attention_bwd(const double* __restrict__ q, const double* __restrict__ k,
                                                           const double* __restrict__ v, const double* __restrict__ P,
                                                           const double* __restrict__ dO, double* __restrict__ dq, double* __restrict__ dk,
                                                           double* __restrict__ dv, int n, int H, int hd, long A) {
  HIP_DYNAMIC_SHARED(char, nucb_smem)
  double* dS = reinterpret_cast<double*>(nucb_smem);
  const long b = blockIdx.x / H;
  const int h = blockIdx.x - (int)b * H, t = threadIdx.x, D = H * hd, c0 = h * hd, S = n + 1;
  const double sc = 1.0 / sqrt((double)hd);
  const double* dOb = dO + b * A;
  if (t < n) {
    const double* Pr = P + ((long)h * n + t) * n;
    double* dSr = dS + t * S;
    double m = 0.0;
    for (int T = 0; T < n; ++T) {
      double p = 0.0;
      for (int d = 0; d < hd; ++d) p += dOb[(long)t * D + c0 + d] * v[(long)T * D + c0 + d];
      dSr[T] = p;
      m += Pr[T] * p;
    }
    for (int T = 0; T < n; ++T) dSr[T] = Pr[T] * (dSr[T] - m);
    for (int d = 0; d < hd; ++d) {
      double a = 0.0;
      for (int T = 0; T < n; ++T) a += dSr[T] * k[(long)T * D + c0 + d];
      dq[b * A + (long)t * D + c0 + d] += sc * a;
    }
  }
  __syncthreads();
  if (t < n) {
    for (int d = 0; d < hd; ++d) {
      double ak = 0.0, av = 0.0;
      for (int tt = 0; tt < n; ++tt) {
        ak += dS[tt * S + t] * q[(long)tt * D + c0 + d];
        av += P[((long)h * n + tt) * n + t] * dOb[(long)tt * D + c0 + d];
      }
      dk[b * A + (long)t * D + c0 + d] += sc * ak;
      dv[b * A + (long)t * D + c0 + d] += av;
    }
  }
}

// table[z + e] = act'(Z[z + e]) for the elements of up to NUC_DACT_JOBS activated layers, concatenated: the derivative depends on
// the SHARED pre-activations alone, so it is evaluated once per call, not once per walker (tanh and exp in double are the
// expensive part of the A operand of k_nucb_dx)
constexpr int NUC_DACT_JOBS = 24;
struct NucDactJobs { int count; int act[NUC_DACT_JOBS]; long z[NUC_DACT_JOBS], n[NUC_DACT_JOBS]; };
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_dact(const double* __restrict__ acts, double* __restrict__ table, NucDactJobs J) {
  long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  for (int j = 0; j < J.count; ++j) {
    if (e < J.n[j]) { table[J.z[j] + e] = nuc_dact(acts[J.z[j] + e], J.act[j]); return; }
    e -= J.n[j];
  }
}

// dX[m][i] += sum_o dY[m][o] act'(Z[rr][o]) W[i][o] for i < k_cols, on v_mfma_f64_16x16x4_f64.  Row m = (b, rr), rr < rows (the
// rows per walker), lives at b * A + rr * width of its arena; dA = act'(Z) [rows][n_out] (k_nucb_dact; nullptr: no activation)
// and W [n_in][n_out] are shared by the walkers.
// A workgroup of four waves stages the panel W[16 CT blockIdx.y ..][:] in the LDS once (row stride S, odd, zero beyond n_out
// and k_cols) and walks its share of the 16-row tiles; a wave holds the CT 16 x 16 tiles of one row tile, so the A operand --
// dY times the activation's derivative, formed while it is loaded, eight k-steps of loads in flight at a time -- is read once
// per panel.  The first panel also writes dZ = dY act'(Z) (a buffer of its own in the arena, what a per-walker weight gradient
// would read).
template <int CT>
__global__ void __launch_bounds__(256) k_nucb_dx(const double* __restrict__ dY, const double* __restrict__ dA, const double* __restrict__ W,
                                                 double* __restrict__ dZ, double* __restrict__ dX, int rows, long M, int n_in, int n_out,
                                                 int k_cols, int S, long A) {
  typedef Mfma<double>::acc_t acc_t;
  HIP_DYNAMIC_SHARED(char, nucb_smem)
  double* Ws = reinterpret_cast<double*>(nucb_smem);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int i0 = blockIdx.y * 16 * CT;
  for (int e = threadIdx.x; e < 16 * CT * S; e += 256) {
    const int c = e / S, o = e - c * S;
    Ws[e] = (i0 + c < k_cols && o < n_out) ? W[(long)(i0 + c) * n_out + o] : 0.0;
  }
  __syncthreads();
  const long n_tiles = (M + 15) / 16;
  for (long tile = (long)blockIdx.x * 4 + wv; tile < n_tiles; tile += (long)gridDim.x * 4) {
    const long ma = tile * 16 + l15;
    const long ba = ma / rows;
    const int ra = (int)(ma - ba * rows);
    const double* yrow = dY + ba * A + (long)ra * n_out;
    const double* drow = dA ? dA + (long)ra * n_out : nullptr;
    double* dzrow = dZ + ba * A + (long)ra * n_out;
    acc_t acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = acc_t{0, 0, 0, 0};
    for (int o0 = 0; o0 < n_out; o0 += 32) {
      double a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = o0 + 4 * j + l4;
        a[j] = (ma < M && o < n_out) ? yrow[o] : 0.0;
      }
      if (dA) {
        double d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int o = o0 + 4 * j + l4;
          d[j] = (ma < M && o < n_out) ? drow[o] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] *= d[j];
        if (blockIdx.y == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int o = o0 + 4 * j + l4;
            if (ma < M && o < n_out) dzrow[o] = a[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (o0 + 4 * j < n_out) {      // (uniform over the wave; the panel's rows are zero-filled up to the next multiple of 4)
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[c] = Mfma<double>::run(a[j], Ws[(c * 16 + l15) * S + o0 + 4 * j + l4], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int i = i0 + c * 16 + l15;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long m = tile * 16 + Mfma<double>::row_of(lane, j);
        if (m < M && i < k_cols) {
          const long b = m / rows;
          dX[b * A + (m - b * rows) * n_in + i] += acc[c][j];
        }
      }
    }
  }
}

// The edge features' adjoint carried into R, added into grad_R (the context's precision) after the electron stream's part.
// With d = R[r] - R[s], rho = sqrt(eps + |d|^2), s(rho) = log1p(rho) / rho the features of edge (s n + r) are F0 = log1p(rho)
// and F_{1+c} = d_c s(rho):  dF0/dd_c = d_c / (rho (1 + rho)),  dF_{1+c}/dd_c' = delta_cc' s + d_c d_c' (1 / (1 + rho) - s) / rho^2.
// The edge's d/dd enters R[r] with + and R[s] with -.  One thread per (walker, nucleus a, component): its 2 n - 2 off-diagonal
// edges in ascending edge order (the diagonal edge cancels).  Walkers with sign 0 or a non-finite log|psi| keep their rows.
template <typename real>
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_edge_feat_bwd(const double* __restrict__ R, double eps, const double* __restrict__ dF,
                                                                  int n, long A, const real* __restrict__ lp, const int32_t* __restrict__ sg,
                                                                  real* __restrict__ grad_R, long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % 3);
  const long q = idx / 3;
  const int a = (int)(q % n);
  const long b = q / n;
  const double l = (double)lp[b];
  if (sg[b] == 0 || !(l - l == 0)) return;
  const int w = 4 + n;
  const double* g = dF + b * A;
  auto edge = [&](int s, int r) {      // d log|psi| / d d_x of edge (s, r)
    const double d[3] = {R[3 * r] - R[3 * s], R[3 * r + 1] - R[3 * s + 1], R[3 * r + 2] - R[3 * s + 2]};
    const double rho = sqrt(eps + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
    const double ir = 1.0 / (1.0 + rho), sc = log1p(rho) / rho;
    const double* ge = g + ((long)s * n + r) * w;
    const double gd = ge[1] * d[0] + ge[2] * d[1] + ge[3] * d[2];
    return ge[0] * d[x] * ir / rho + ge[1 + x] * sc + d[x] * gd * (ir - sc) / (rho * rho);
  };
  double acc = 0.0;
  for (int s = 0; s < n; ++s) {
    if (s != a) acc += edge(s, a);
    else for (int r = 0; r < n; ++r) if (r != a) acc -= edge(a, r);
  }
  grad_R[idx] += (real)acc;
}

// ---- option "nuclear_params": the stream's parameter partials per walker (engine_nuc.inl: nuc_fold_rows) ----
// dW_b[i][o] = sum_r X[r][i] dZ_b[r][o] (i < n_in) and, as row n_in of the same product against a column of ones, the bias
// partial db_b[o] = sum_r dZ_b[r][o], on v_mfma_f64_16x16x4_f64.  X [rows][n_in] is shared by the walkers, walker b's dZ
// [rows][n_out] lives at dZ + b * A (its adjoint arena).  The contraction runs over the rows, zero-padded to a multiple of 4.
// A workgroup of four waves stages the tile X^T[16 blockIdx.x ..][:] in the LDS once (row stride S, odd, zeros beyond rows and
// n_in, ones in the bias row) and walks over its slice of the walkers, blockIdx.z of gridDim.z contiguous slices; wave wv owns
// the 16 output columns of tile 4 blockIdx.y + wv.  A walker's tile is a sum in the fixed order of the MFMA's k-steps and does
// not depend on the other walkers.  Two epilogues:
//   SQ false  the tile is ADDED to row b of out [B][ld] at w_off + i n_out + o (theta order), the bias row at b_off + o;
//   SQ true   the squares of the tile's elements are summed over the slice's walkers in ascending order and written to
//             part[blockIdx.z][E], E = (n_in + 1) n_out (the bias row last): no per-walker row exists, nothing is added
//             concurrently; k_nucb_sqsum combines the slices in ascending order.
template <bool SQ, typename real>
__global__ void __launch_bounds__(256) k_nucb_dw(const double* __restrict__ X, const double* __restrict__ dZ, long A, int rows, int n_in,
                                                 int n_out, int has_bias, int B, int S, real* __restrict__ out, long ld, long w_off,
                                                 long b_off, double* __restrict__ part) {
  typedef Mfma<double>::acc_t acc_t;
  HIP_DYNAMIC_SHARED(char, nucb_smem)
  double* Xs = reinterpret_cast<double*>(nucb_smem);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int i0 = blockIdx.x * 16, rows4 = (rows + 3) / 4 * 4;
  for (int e = threadIdx.x; e < 16 * S; e += 256) {
    const int c = e / S, r = e - c * S, i = i0 + c;
    double x = 0.0;
    if (r < rows) x = i < n_in ? X[(long)r * n_in + i] : (i == n_in && has_bias) ? 1.0 : 0.0;
    Xs[e] = x;
  }
  __syncthreads();
  const int o = (blockIdx.y * 4 + wv) * 16 + l15;
  if ((blockIdx.y * 4 + wv) * 16 >= n_out) return;      // (uniform over the wave; no barrier follows)
  const int per = (B + (int)gridDim.z - 1) / (int)gridDim.z;
  const int b_lo = (int)blockIdx.z * per, b_hi = b_lo + per < B ? b_lo + per : B;
  double sq[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = b_lo; b < b_hi; ++b) {
    const double* z = dZ + (long)b * A;
    acc_t acc = acc_t{0, 0, 0, 0};
    for (int k0 = 0; k0 < rows4; k0 += 4) {
      const int r = k0 + l4;
      const double bv = (r < rows && o < n_out) ? z[(long)r * n_out + o] : 0.0;
      acc = Mfma<double>::run(Xs[l15 * S + r], bv, acc);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (SQ) {
        sq[j] += acc[j] * acc[j];
      } else {
        const int i = i0 + Mfma<double>::row_of(lane, j);
        if (o < n_out) {
          if (i < n_in) out[(long)b * ld + w_off + (long)i * n_out + o] += (real)acc[j];
          else if (i == n_in && has_bias) out[(long)b * ld + b_off + o] += (real)acc[j];
        }
      }
    }
  }
  if constexpr (SQ) {
    const long E = (long)(n_in + 1) * n_out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + Mfma<double>::row_of(lane, j);
      if (o < n_out && i <= n_in) part[(long)blockIdx.z * E + (long)i * n_out + o] = sq[j];
    }
  }
}
// F[w_off + e] += sum_z part[z][e] (e < n_in n_out), F[b_off + e - n_in n_out] likewise for the bias row, z ascending
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_sqsum(const double* __restrict__ part, int nz, int n_in, int n_out, int has_bias,
                                                          double* __restrict__ F, long w_off, long b_off) {
  const long e = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  const long nw = (long)n_in * n_out, E = nw + n_out;
  if (e >= (has_bias ? E : nw)) return;
  double s = 0.0;
  for (int z = 0; z < nz; ++z) s += part[(long)z * E + e];
  F[e < nw ? w_off + e : b_off + (e - nw)] += s;
}
// the zeta tables' bias: walker b's partial is its adjoint of the table, dzeta + b * A.  SQ false: out[b][off + e] += it;
// SQ true: F[off + e] += the sum of its squares over the walkers, ascending
template <bool SQ, typename real>
__global__ void __launch_bounds__(NUC_BLOCK) k_nucb_zbias(const double* __restrict__ dzeta, long A, long n, int B, real* __restrict__ out,
                                                          long ld, long off, double* __restrict__ F) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if constexpr (SQ) {
    if (idx >= n) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) { const double v = dzeta[(long)b * A + idx]; s += v * v; }
    F[off + idx] += s;
  } else {
    if (idx >= n * B) return;
    const long b = idx / n, e = idx - b * n;
    out[b * ld + off + e] += (real)dzeta[b * A + e];
  }
}
// Row b of jt [B][ld_t] = the transpose of the packing applied to row b of jac [B][ld_jac]: element p sums its copies
// jac[b][col], ascending, in the context's precision.  Rows of walkers with sign 0 or a non-finite log|psi| are zero.
template <typename real>
__global__ void __launch_bounds__(NUC_BLOCK) k_jac_to_params(const real* __restrict__ jac, long ld_jac, const int32_t* __restrict__ row,
                                                             const int32_t* __restrict__ col, const real* __restrict__ lp,
                                                             const int32_t* __restrict__ sg, real* __restrict__ jt, long ld_t, long n_params,
                                                             long total) {
  const long idx = (long)blockIdx.x * NUC_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / n_params, p = idx - b * n_params;
  const double l = (double)lp[b];
  real s = 0;
  if (sg[b] != 0 && l - l == 0)
    for (int32_t k = row[p]; k < row[p + 1]; ++k) s += jac[b * ld_jac + col[k]];
  jt[b * ld_t + p] = s;
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

template <typename T>
void launch_nucb_gather(hipStream_t st, const T* src, long stride, long w0, long len, const int32_t* row, const int32_t* col, long e_lo,
                        long e_hi, double* G, long A, int B) {
  const long total = (long)B * (e_hi - e_lo);
  if (total <= 0) return;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_gather<T>), dim3(nuc_grid(total)), dim3(NUC_BLOCK), 0, st, src, stride, w0, len, row, col, e_lo,
                     e_hi, G, A, total);
}
template void launch_nucb_gather<float>(hipStream_t, const float*, long, long, long, const int32_t*, const int32_t*, long, long, double*, long, int);
template void launch_nucb_gather<double>(hipStream_t, const double*, long, long, long, const int32_t*, const int32_t*, long, long, double*, long,
                                         int);
void launch_nucb_add(hipStream_t st, double* a, const double* c, long n, long A, int B) {
  hipLaunchKernelGGL(k_nucb_add, dim3(nuc_grid(n * B)), dim3(NUC_BLOCK), 0, st, a, c, n, A, n * B);
}
void launch_nucb_glu_bwd(hipStream_t st, const double* zw, const double* zv, const double* dzeta, double* dzw, double* dzv, long n, long A,
                         int B) {
  hipLaunchKernelGGL(k_nucb_glu_bwd, dim3(nuc_grid(n * B)), dim3(NUC_BLOCK), 0, st, zw, zv, dzeta, dzw, dzv, n, A, n * B);
}
void launch_nucb_layernorm_bwd(hipStream_t st, const double* ln, const double* rstd, const double* dln, double* dh, int n, int D, long A,
                               int B) {
  const long total = (long)n * B;
  hipLaunchKernelGGL(k_nucb_layernorm_bwd, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, ln, rstd, dln, dh, n, D, A, total);
}
void launch_nucb_sender_sum_bwd(hipStream_t st, const double* dout, double* din, int n, int w, long A, int B) {
  const long total = (long)n * n * w * B;
  hipLaunchKernelGGL(k_nucb_sender_sum_bwd, dim3(nuc_grid(total)), dim3(NUC_BLOCK), 0, st, dout, din, n, w, A, total);
}
size_t nucb_attention_bwd_lds_bytes(int n) { return sizeof(double) * (size_t)n * (n + 1); }
void launch_nucb_attention_bwd(hipStream_t st, const double* q, const double* k, const double* v, const double* P, const double* dO,
                               double* dq, double* dk, double* dv, int n, int H, int hd, long A, int B) {
  hipLaunchKernelGGL(k_nucb_attention_bwd, dim3((unsigned)((long)B * H)), dim3(64), nucb_attention_bwd_lds_bytes(n), st, q, k, v, P, dO, dq, dk,
                     dv, n, H, hd, A);
}
// column tiles per workgroup of k_nucb_dx for a panel of k_cols columns and n_out deep: the widest of 4, 2, 1 (no wider than
// the columns need) whose panel leaves room for two workgroups per CU (80 KB), else the widest that fits the 160 KB of a CU
// at all; 0: none does
static inline int nucb_dx_row_stride(int n_out) { return ((n_out + 3) / 4 * 4) | 1; }
size_t nucb_dx_lds_bytes(int ct, int n_out) { return sizeof(double) * 16 * (size_t)ct * nucb_dx_row_stride(n_out); }
int nucb_dx_col_tiles(int k_cols, int n_out) {
  const int need = (k_cols + 15) / 16;
  for (int ct = 4; ct >= 1; ct >>= 1)
    if ((ct == 1 || ct / 2 < need) && nucb_dx_lds_bytes(ct, n_out) <= (size_t)80 * 1024) return ct;
  for (int ct = 4; ct >= 1; ct >>= 1)
    if ((ct == 1 || ct / 2 < need) && nucb_dx_lds_bytes(ct, n_out) <= (size_t)160 * 1024) return ct;
  return 0;
}
void launch_nucb_dact(hipStream_t st, const double* acts, double* table, const int* act, const long* z, const long* n, int count) {
  for (int j0 = 0; j0 < count; j0 += NUC_DACT_JOBS) {
    NucDactJobs J{};
    long total = 0;
    J.count = count - j0 < NUC_DACT_JOBS ? count - j0 : NUC_DACT_JOBS;
    for (int j = 0; j < J.count; ++j) { J.act[j] = act[j0 + j]; J.z[j] = z[j0 + j]; J.n[j] = n[j0 + j]; total += n[j0 + j]; }
    if (total > 0) hipLaunchKernelGGL(k_nucb_dact, dim3(nuc_grid(total)), dim3(NUC_BLOCK), 0, st, acts, table, J);
  }
}
template <int CT>
static int nucb_dx_launch(hipStream_t st, const double* dY, const double* dA, const double* W, double* dZ, double* dX, int rows, long M,
                          int n_in, int n_out, int k_cols, long A) {
  const size_t lds = nucb_dx_lds_bytes(CT, n_out);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nucb_dx<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -2;
  const long groups = ((M + 15) / 16 + 3) / 4;
  const unsigned gx = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_dx<CT>), dim3(gx, (unsigned)((k_cols + 16 * CT - 1) / (16 * CT))), dim3(256), lds, st, dY, dA, W, dZ,
                     dX, rows, M, n_in, n_out, k_cols, nucb_dx_row_stride(n_out), A);
  return 0;
}
int launch_nucb_dx(hipStream_t st, const double* dY, const double* dA, const double* W, double* dZ, double* dX, int rows, int B, int n_in,
                   int n_out, int k_cols, long A) {
  const long M = (long)B * rows;
  switch (nucb_dx_col_tiles(k_cols, n_out)) {
    case 4: return nucb_dx_launch<4>(st, dY, dA, W, dZ, dX, rows, M, n_in, n_out, k_cols, A);
    case 2: return nucb_dx_launch<2>(st, dY, dA, W, dZ, dX, rows, M, n_in, n_out, k_cols, A);
    case 1: return nucb_dx_launch<1>(st, dY, dA, W, dZ, dX, rows, M, n_in, n_out, k_cols, A);
    default: return -1;
  }
}
template <typename real>
void launch_nucb_edge_feat_bwd(hipStream_t st, const double* R, double eps, const double* dF, int n, long A, const real* lp, const int32_t* sg,
                               real* grad_R, int B) {
  const long total = (long)B * n * 3;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_edge_feat_bwd<real>), dim3(nuc_grid(total)), dim3(NUC_BLOCK), 0, st, R, eps, dF, n, A, lp, sg,
                     grad_R, total);
}
template void launch_nucb_edge_feat_bwd<float>(hipStream_t, const double*, double, const double*, int, long, const float*, const int32_t*,
                                               float*, int);
template void launch_nucb_edge_feat_bwd<double>(hipStream_t, const double*, double, const double*, int, long, const double*, const int32_t*,
                                                double*, int);

static inline int nucb_dw_row_stride(int rows) { return ((rows + 3) / 4 * 4) | 1; }
size_t nucb_dw_lds_bytes(int rows) { return sizeof(double) * 16 * (size_t)nucb_dw_row_stride(rows); }
bool nucb_dw_fits(int rows) { return nucb_dw_lds_bytes(rows) <= (size_t)160 * 1024; }
int nucb_dw_slices(int B) { return B < NUCB_DW_SLICES ? B : NUCB_DW_SLICES; }
size_t nucb_dw_part_doubles(int n_in, int n_out) { return (size_t)NUCB_DW_SLICES * (size_t)(n_in + 1) * n_out; }
template <bool SQ, typename real>
static int nucb_dw_launch(hipStream_t st, const double* X, const double* dZ, long A, int rows, int n_in, int n_out, int has_bias, int B,
                          real* out, long ld, long w_off, long b_off, double* part) {
  const size_t lds = nucb_dw_lds_bytes(rows);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nucb_dw<SQ, real>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -2;
  const dim3 grid((unsigned)((n_in + (has_bias ? 1 : 0) + 15) / 16), (unsigned)((n_out + 63) / 64), (unsigned)nucb_dw_slices(B));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_dw<SQ, real>), grid, dim3(256), lds, st, X, dZ, A, rows, n_in, n_out, has_bias, B,
                     nucb_dw_row_stride(rows), out, ld, w_off, b_off, part);
  return 0;
}
template <typename real>
int launch_nucb_dw_store(hipStream_t st, const double* X, const double* dZ, long A, int rows, int n_in, int n_out, int B, real* out, long ld,
                         long w_off, long b_off) {
  if (!nucb_dw_fits(rows)) return -1;
  return nucb_dw_launch<false, real>(st, X, dZ, A, rows, n_in, n_out, b_off >= 0 ? 1 : 0, B, out, ld, w_off, b_off, nullptr);
}
template int launch_nucb_dw_store<float>(hipStream_t, const double*, const double*, long, int, int, int, int, float*, long, long, long);
template int launch_nucb_dw_store<double>(hipStream_t, const double*, const double*, long, int, int, int, int, double*, long, long, long);
int launch_nucb_dw_sqsum(hipStream_t st, const double* X, const double* dZ, long A, int rows, int n_in, int n_out, int B, double* F,
                         long w_off, long b_off, double* part) {
  if (!nucb_dw_fits(rows)) return -1;
  const int hb = b_off >= 0 ? 1 : 0;
  const int rc = nucb_dw_launch<true, double>(st, X, dZ, A, rows, n_in, n_out, hb, B, nullptr, 0, w_off, b_off, part);
  if (rc) return rc;
  hipLaunchKernelGGL(k_nucb_sqsum, dim3(nuc_grid((long)(n_in + 1) * n_out)), dim3(NUC_BLOCK), 0, st, part, nucb_dw_slices(B), n_in, n_out, hb,
                     F, w_off, b_off);
  return 0;
}
template <typename real>
void launch_nucb_zbias_store(hipStream_t st, const double* dzeta, long A, long n, int B, real* out, long ld, long off) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_zbias<false, real>), dim3(nuc_grid(n * B)), dim3(NUC_BLOCK), 0, st, dzeta, A, n, B, out, ld, off,
                     nullptr);
}
template void launch_nucb_zbias_store<float>(hipStream_t, const double*, long, long, int, float*, long, long);
template void launch_nucb_zbias_store<double>(hipStream_t, const double*, long, long, int, double*, long, long);
void launch_nucb_zbias_sqsum(hipStream_t st, const double* dzeta, long A, long n, int B, double* F, long off) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nucb_zbias<true, double>), dim3(nuc_grid(n)), dim3(NUC_BLOCK), 0, st, dzeta, A, n, B, nullptr, 0, off, F);
}
template <typename real>
void launch_jac_to_params(hipStream_t st, const real* jac, long ld_jac, const int32_t* row, const int32_t* col, const real* lp,
                          const int32_t* sg, real* jt, long ld_t, long n_params, int B) {
  const long total = n_params * B;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_to_params<real>), dim3(nuc_grid(total)), dim3(NUC_BLOCK), 0, st, jac, ld_jac, row, col, lp, sg, jt,
                     ld_t, n_params, total);
}
template void launch_jac_to_params<float>(hipStream_t, const float*, long, const int32_t*, const int32_t*, const float*, const int32_t*, float*,
                                          long, long, int);
template void launch_jac_to_params<double>(hipStream_t, const double*, long, const int32_t*, const int32_t*, const double*, const int32_t*,
                                           double*, long, long, int);
