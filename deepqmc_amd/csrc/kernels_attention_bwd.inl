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
//
// NC (the nuclear tokens of the TransPsiformer, option "nuclear_reverse"): n_const further key / value rows kc, vc
// [n_const][H * hd] that all walkers share.  As in the forward they come FIRST in the key order (M = n_const + N keys), so the
// row maximum and the row sum of the softmax run over them before the electrons.  They have no adjoint buffer: the (walker,
// head) partials dKc, dVc go to cpart[b][2][n_const][H * hd], every element written by exactly one thread of one workgroup,
// and the engine sums them over the walkers with its fixed-order column sum.  Their accumulators are registers of their own
// (ATT_BWD_EPT_C per thread), so the ownership limit of the electron rows is the one of NC = false.  NC = false compiles to
// the kernel without any of this: the same sums in the same order.

constexpr int ATT_BWD_QB = 16;       // query rows per block
constexpr int ATT_BWD_EPT = 16;      // dk / dv elements per thread: N * hd <= ATT_BWD_EPT * blockDim.x
constexpr int ATT_BWD_EPT_C = 16;    // dKc / dVc elements per thread: n_const * hd <= ATT_BWD_EPT_C * blockDim.x

template <typename real, bool NC>
__global__ void __launch_bounds__(256) k_attention_bwd(const real* __restrict__ q, const real* __restrict__ k,
                                                       const real* __restrict__ v, const real* __restrict__ dout,
                                                       real* __restrict__ dq, real* __restrict__ dk, real* __restrict__ dv,
                                                       int width, int H, int hd, int N, int n_const,
                                                       const real* __restrict__ kc, const real* __restrict__ vc,
                                                       real* __restrict__ cpart) {
  HIP_DYNAMIC_SHARED(char, smem_raw)
  real* sm = reinterpret_cast<real*>(smem_raw);
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int S = hd + 1;              // padded row stride of the [rows][hd] tiles
  const int QB = N < ATT_BWD_QB ? N : ATT_BWD_QB;
  const int NH = N * hd;
  const int nc = NC ? n_const : 0, M = nc + N, NCH = nc * hd;   // keys: the constant rows first, then the electrons
  real* kt = sm;            real* vt = kt + M * S;          // [M][S]
  real* qb = vt + M * S;    real* gb = qb + QB * S;         // [QB][S]: q and dO rows of the block
  real* P = gb + QB * S;    real* dS = P + QB * M;          // [QB][M]
  real* mrow = dS + QB * M;                                 // [QB]
  const real sc = (real)(1.0 / sqrt((double)hd));
  const long row0 = (long)b * N;
  const int col0 = h * hd;

  if (NC)
    for (int e = tid; e < NCH; e += nthr) {
      const int j = e / hd, d = e - j * hd;
      kt[j * S + d] = kc[(long)j * (H * hd) + col0 + d];
      vt[j * S + d] = vc[(long)j * (H * hd) + col0 + d];
    }
  for (int e = tid; e < NH; e += nthr) {
    const int j = e / hd, d = e - j * hd;
    kt[(nc + j) * S + d] = k[(row0 + j) * width + col0 + d];
    vt[(nc + j) * S + d] = v[(row0 + j) * width + col0 + d];
  }
  real acc_k[ATT_BWD_EPT], acc_v[ATT_BWD_EPT];
#pragma unroll
  for (int c = 0; c < ATT_BWD_EPT; ++c) { acc_k[c] = 0; acc_v[c] = 0; }
  real acc_kc[NC ? ATT_BWD_EPT_C : 1], acc_vc[NC ? ATT_BWD_EPT_C : 1];
  if (NC) {
#pragma unroll
    for (int c = 0; c < ATT_BWD_EPT_C; ++c) { acc_kc[c] = 0; acc_vc[c] = 0; }
  }

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
    for (int e = tid; e < nq * M; e += nthr) {
      const int i = e / M, j = e - i * M;
      real s = 0, p = 0;
      for (int d = 0; d < hd; ++d) { s += qb[i * S + d] * kt[j * S + d]; p += gb[i * S + d] * vt[j * S + d]; }
      P[e] = s * sc;
      dS[e] = p;
    }
    __syncthreads();
    // softmax over the keys as the forward forms it, and m_i = sum_j P_ij dP_ij
    if (tid < nq) {
      real* Pr = P + tid * M;
      const real* dPr = dS + tid * M;
      real mx = Pr[0];
      for (int j = 1; j < M; ++j) mx = Pr[j] > mx ? Pr[j] : mx;
      real sum = 0;
      for (int j = 0; j < M; ++j) { const real ev = r_exp<real>(Pr[j] - mx); Pr[j] = ev; sum += ev; }
      const real inv = 1 / sum;
      real m = 0;
      for (int j = 0; j < M; ++j) { Pr[j] *= inv; m += Pr[j] * dPr[j]; }
      mrow[tid] = m;
    }
    __syncthreads();
    for (int e = tid; e < nq * M; e += nthr) dS[e] = P[e] * (dS[e] - mrow[e / M]);
    __syncthreads();
    // dq of the block's rows: each element belongs to one thread of one workgroup
    for (int e = tid; e < nq * hd; e += nthr) {
      const int i = e / hd, d = e - i * hd;
      real a = 0;
      for (int j = 0; j < M; ++j) a += dS[i * M + j] * kt[j * S + d];
      dq[(row0 + i0 + i) * width + col0 + d] += sc * a;
    }
    // dk, dv: this block's query rows added to the thread's register elements
#pragma unroll
    for (int c = 0; c < ATT_BWD_EPT; ++c) {
      const int e = c * nthr + tid;
      if (e < NH) {
        const int j = e / hd, d = e - j * hd;
        real ak = acc_k[c], av = acc_v[c];
        for (int i = 0; i < nq; ++i) { ak += dS[i * M + nc + j] * qb[i * S + d]; av += P[i * M + nc + j] * gb[i * S + d]; }
        acc_k[c] = ak; acc_v[c] = av;
      }
    }
    if (NC) {
#pragma unroll
      for (int c = 0; c < ATT_BWD_EPT_C; ++c) {
        const int e = c * nthr + tid;
        if (e < NCH) {
          const int j = e / hd, d = e - j * hd;
          real ak = acc_kc[c], av = acc_vc[c];
          for (int i = 0; i < nq; ++i) { ak += dS[i * M + j] * qb[i * S + d]; av += P[i * M + j] * gb[i * S + d]; }
          acc_kc[c] = ak; acc_vc[c] = av;
        }
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
  if (NC) {
    const long HD = (long)H * hd;
    real* pk = cpart + (long)b * 2 * nc * HD;
#pragma unroll
    for (int c = 0; c < ATT_BWD_EPT_C; ++c) {
      const int e = c * nthr + tid;
      if (e < NCH) {
        const int j = e / hd, d = e - j * hd;
        pk[j * HD + col0 + d] = sc * acc_kc[c];
        pk[(nc + j) * HD + col0 + d] = acc_vc[c];
      }
    }
  }
}

template <typename real> size_t attention_bwd_lds_bytes(int N, int hd, int n_const) {
  const size_t QB = N < ATT_BWD_QB ? N : ATT_BWD_QB, M = (size_t)N + n_const;
  return sizeof(real) * ((2 * M + 2 * QB) * (hd + 1) + 2 * QB * M + QB);
}

template <typename real, bool NC>
static int launch_attention_bwd_nc(hipStream_t st, const real* q, const real* k, const real* v, const real* dout, real* dq, real* dk,
                                   real* dv, int width, int H, int hd, int B, int N, int n_const, const real* kc, const real* vc,
                                   real* cpart) {
  // few keys: one wave per (walker, head), as the forward
  const unsigned nthr = N + n_const <= 8 ? 64u : 256u;
  const size_t lds = attention_bwd_lds_bytes<real>(N, hd, n_const);
  if (lds > (size_t)160 * 1024 || (size_t)N * hd > (size_t)ATT_BWD_EPT * nthr || (size_t)n_const * hd > (size_t)ATT_BWD_EPT_C * nthr) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_bwd<real, NC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return -2;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_attention_bwd<real, NC>), dim3((unsigned)(B * H)), dim3(nthr), lds, st, q, k, v, dout, dq, dk, dv,
                     width, H, hd, N, n_const, kc, vc, cpart);
  return 0;
}

// n_const > 0: kc, vc [n_const][H * hd] and cpart [B][2][n_const][H * hd] must be given
template <typename real>
int launch_attention_bwd(hipStream_t st, const real* q, const real* k, const real* v, const real* dout, real* dq, real* dk, real* dv,
                         int width, int H, int hd, int B, int N, int n_const, const real* kc, const real* vc, real* cpart) {
  if (B < 1 || H < 1 || hd < 1 || N < 1 || width < H * hd || n_const < 0) return -1;
  if (n_const > 0) {
    if (!kc || !vc || !cpart) return -1;
    return launch_attention_bwd_nc<real, true>(st, q, k, v, dout, dq, dk, dv, width, H, hd, B, N, n_const, kc, vc, cpart);
  }
  return launch_attention_bwd_nc<real, false>(st, q, k, v, dout, dq, dk, dv, width, H, hd, B, N, 0, nullptr, nullptr, nullptr);
}

template size_t attention_bwd_lds_bytes<float>(int, int, int);
template size_t attention_bwd_lds_bytes<double>(int, int, int);
template int launch_attention_bwd<float>(hipStream_t, const float*, const float*, const float*, const float*, float*, float*, float*, int,
                                         int, int, int, int, int, const float*, const float*, float*);
template int launch_attention_bwd<double>(hipStream_t, const double*, const double*, const double*, const double*, double*, double*,
                                          double*, int, int, int, int, int, int, const double*, const double*, double*);
