// kernels_attention_bwd.inl -- included by kernel_attention.hip (inside namespace dqmc): the value-level backward of the
// attention op for the reverse pass of log|psi| (engine_reverse.inl, every mode; the op has no parameters).
//
// Per (walker, head), with S = s q k^T, s = 1/sqrt(hd), P = row-softmax(S), O = P v and the adjoint dO of O:
//   dv = P^T dO,   dP = dO v^T,   dS_ij = P_ij (dP_ij - sum_j' P_ij' dP_ij'),   dq = s dS k,   dk = s dS^T q.
// P is recomputed from q and k (nothing is stored by the forward); dq, dk, dv are ADDED into the adjoint buffers.
//
// One workgroup per (walker, head): no two workgroups touch the same adjoint element, so there are no atomics and every sum
// runs in a fixed order (keys and features ascending, query rows ascending across the blocks).  k and v stay in LDS with
// the forward's padded row stride; the queries go through in blocks of ATT_BWD_QB rows with their q, dO, P and dS tiles in
// LDS (all of them resident would need 165 KB in float64 at N = hd = 64).  Each thread owns up to ATT_BWD_EPT fixed (key,
// feature) elements of dk and dv in registers across the blocks and adds them to memory once at the end.
// Layout as k_attention with TP = 1: row b * N + i, columns h * hd .. h * hd + hd - 1, row stride `width`.

constexpr int ATT_BWD_QB = 16;       // query rows per block
constexpr int ATT_BWD_EPT = 16;      // dk / dv elements per thread: N * hd <= ATT_BWD_EPT * blockDim.x

template <typename real>
__global__ void __launch_bounds__(256) k_attention_bwd(const real* __restrict__ q, const real* __restrict__ k,
                                                       const real* __restrict__ v, const real* __restrict__ dout,
                                                       real* __restrict__ dq, real* __restrict__ dk, real* __restrict__ dv,
                                                       int width, int H, int hd, int N) {
  HIP_DYNAMIC_SHARED(char, smem_raw)
  real* sm = reinterpret_cast<real*>(smem_raw);
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int S = hd + 1;              // padded row stride of the [rows][hd] tiles
  const int QB = N < ATT_BWD_QB ? N : ATT_BWD_QB;
  const int NH = N * hd;
  real* kt = sm;            real* vt = kt + N * S;          // [N][S]
  real* qb = vt + N * S;    real* gb = qb + QB * S;         // [QB][S]: q and dO rows of the block
  real* P = gb + QB * S;    real* dS = P + QB * N;          // [QB][N]
  real* mrow = dS + QB * N;                                 // [QB]
  const real sc = (real)(1.0 / sqrt((double)hd));
  const long row0 = (long)b * N;
  const int col0 = h * hd;

  for (int e = tid; e < NH; e += nthr) {
    const int j = e / hd, d = e - j * hd;
    kt[j * S + d] = k[(row0 + j) * width + col0 + d];
    vt[j * S + d] = v[(row0 + j) * width + col0 + d];
  }
  real acc_k[ATT_BWD_EPT], acc_v[ATT_BWD_EPT];
#pragma unroll
  for (int c = 0; c < ATT_BWD_EPT; ++c) { acc_k[c] = 0; acc_v[c] = 0; }

  for (int i0 = 0; i0 < N; i0 += QB) {
    const int nq = (N - i0) < QB ? (N - i0) : QB;
    __syncthreads();                 // the previous block's tiles are no longer read (first block: kt, vt are complete below)
    for (int e = tid; e < nq * hd; e += nthr) {
      const int i = e / hd, d = e - i * hd;
      qb[i * S + d] = q[(row0 + i0 + i) * width + col0 + d];
      gb[i * S + d] = dout[(row0 + i0 + i) * width + col0 + d];
    }
    __syncthreads();
    // logits and dP = dO v^T
    for (int e = tid; e < nq * N; e += nthr) {
      const int i = e / N, j = e - i * N;
      real s = 0, p = 0;
      for (int d = 0; d < hd; ++d) { s += qb[i * S + d] * kt[j * S + d]; p += gb[i * S + d] * vt[j * S + d]; }
      P[e] = s * sc;
      dS[e] = p;
    }
    __syncthreads();
    // softmax over the keys as the forward forms it, and m_i = sum_j P_ij dP_ij
    if (tid < nq) {
      real* Pr = P + tid * N;
      const real* dPr = dS + tid * N;
      real mx = Pr[0];
      for (int j = 1; j < N; ++j) mx = Pr[j] > mx ? Pr[j] : mx;
      real sum = 0;
      for (int j = 0; j < N; ++j) { const real ev = r_exp<real>(Pr[j] - mx); Pr[j] = ev; sum += ev; }
      const real inv = 1 / sum;
      real m = 0;
      for (int j = 0; j < N; ++j) { Pr[j] *= inv; m += Pr[j] * dPr[j]; }
      mrow[tid] = m;
    }
    __syncthreads();
    for (int e = tid; e < nq * N; e += nthr) dS[e] = P[e] * (dS[e] - mrow[e / N]);
    __syncthreads();
    // dq of the block's rows: each element belongs to one thread of one workgroup
    for (int e = tid; e < nq * hd; e += nthr) {
      const int i = e / hd, d = e - i * hd;
      real a = 0;
      for (int j = 0; j < N; ++j) a += dS[i * N + j] * kt[j * S + d];
      dq[(row0 + i0 + i) * width + col0 + d] += sc * a;
    }
    // dk, dv: this block's query rows added to the thread's register elements
#pragma unroll
    for (int c = 0; c < ATT_BWD_EPT; ++c) {
      const int e = c * nthr + tid;
      if (e < NH) {
        const int j = e / hd, d = e - j * hd;
        real ak = acc_k[c], av = acc_v[c];
        for (int i = 0; i < nq; ++i) { ak += dS[i * N + j] * qb[i * S + d]; av += P[i * N + j] * gb[i * S + d]; }
        acc_k[c] = ak; acc_v[c] = av;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < ATT_BWD_EPT; ++c) {
    const int e = c * nthr + tid;
    if (e < NH) {
      const int j = e / hd, d = e - j * hd;
      dk[(row0 + j) * width + col0 + d] += sc * acc_k[c];
      dv[(row0 + j) * width + col0 + d] += acc_v[c];
    }
  }
}

template <typename real> size_t attention_bwd_lds_bytes(int N, int hd) {
  const size_t QB = N < ATT_BWD_QB ? N : ATT_BWD_QB;
  return sizeof(real) * (((size_t)2 * N + 2 * QB) * (hd + 1) + 2 * QB * N + QB);
}

template <typename real>
int launch_attention_bwd(hipStream_t st, const real* q, const real* k, const real* v, const real* dout, real* dq, real* dk, real* dv,
                         int width, int H, int hd, int B, int N) {
  if (B < 1 || H < 1 || hd < 1 || N < 1 || width < H * hd) return -1;
  // few electrons: one wave per (walker, head), as the forward
  const unsigned nthr = N <= 8 ? 64u : 256u;
  const size_t lds = attention_bwd_lds_bytes<real>(N, hd);
  if (lds > (size_t)160 * 1024 || (size_t)N * hd > (size_t)ATT_BWD_EPT * nthr) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_bwd<real>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return -2;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_attention_bwd<real>), dim3((unsigned)(B * H)), dim3(nthr), lds, st, q, k, v, dout, dq, dk, dv, width,
                     H, hd, N);
  return 0;
}

template size_t attention_bwd_lds_bytes<float>(int, int);
template size_t attention_bwd_lds_bytes<double>(int, int);
template int launch_attention_bwd<float>(hipStream_t, const float*, const float*, const float*, const float*, float*, float*, float*, int,
                                         int, int, int, int);
template int launch_attention_bwd<double>(hipStream_t, const double*, const double*, const double*, const double*, double*, double*,
                                          double*, int, int, int, int, int);
