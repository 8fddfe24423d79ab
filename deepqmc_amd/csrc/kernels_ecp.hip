// kernels_ecp.hip -- non-local part of Gaussian-type effective core potentials.
//
// Reference: ecp/gaussian_type_ecp.py:161-255 (`nonloc_potential`) + ecp/ecp_utils.py:23-95.
//   V_nl = sum_{a in ecp} sum_i sum_l (2l+1)/12 * V_l(|r_i - R_a|) * sum_{q=1..12} P_l(cos theta_q) psi(r_i -> x_q)/psi(r)
// with x_q the 12 vertices of an icosahedron of radius |r_i - R_a| around R_a, its pole rotated onto the
// electron-nucleus axis and the whole turned about that axis by a random angle in [0, pi/5).
// The 12 N n_ecp value-only psi evaluations per walker are what costs (229 GFLOP/walker for benzene,
// SURVEY.md section 8); they run through the ordinary value path on a batch of "quadrature walkers"
// that k_ecp_points writes, and k_ecp_reduce folds the psi ratios back into E_loc.
// The local part (gaussian_type_ecp.py:127-159) lives in k_final next to the Coulomb terms.
// Further down: the mixed-precision quadrature of float32 contexts, the Hellmann-Feynman force of an ECP Hamiltonian
// (gradient of the local and non-local terms with respect to the nuclei, dqmc_ecp_force) and the pseudo-Hamiltonian.
#include "common.h"
#include "kernels.h"

namespace dqmc {

// cos(theta_q) of the unit icosahedron of ecp_utils.py:23-32: poles, then alternating
// atan(2) / pi - atan(2) rings.
__device__ __forceinline__ double ico_cos(int q) {
  if (q == 0) return 1.0;
  if (q == 1) return -1.0;
  return (q & 1) ? -0.44721359549995793 : 0.44721359549995793;   // -+ 1/sqrt(5)
}
__device__ __forceinline__ double ico_phi(int q) {
  if (q < 2) return 0.0;
  const int j = (q - 2) >> 1;
  return 0.62831853071795865 * ((q & 1) ? (2 * j - 1) : (2 * j));  // pi/5 * ...
}

// Quadrature walkers of the chunk [b0, b0 + nb): config ((bl*n_nl + j)*N + i)*12 + q is walker b0+bl
// with electron i moved to vertex q around nucleus nl_nuc[j].  One thread per coordinate.
template <typename real>
__global__ void __launch_bounds__(256) k_ecp_points(const EcpArgs a, real* __restrict__ rq) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.N;
  const long per_cfg = (long)N * 3;
  const long n_cfg = (long)a.nb * a.n_nl * N * 12;
  if (idx >= n_cfg * per_cfg) return;
  const long cfg = idx / per_cfg;
  const int ec = (int)(idx - cfg * per_cfg), e = ec / 3, c = ec - 3 * e;
  const int q = (int)(cfg % 12);
  const long t1 = cfg / 12;
  const int i = (int)(t1 % N);
  const long t2 = t1 / N;
  const int j = (int)(t2 % a.n_nl), bl = (int)(t2 / a.n_nl);
  const int b = a.b0 + bl;
  const real* r = reinterpret_cast<const real*>(a.r) + (long)b * per_cfg;
  if (e != i) { rq[idx] = r[ec]; return; }
  const real* R = reinterpret_cast<const real*>(a.R) + 3 * a.nl_nuc[j];
  const double dx = (double)r[3 * i] - (double)R[0], dy = (double)r[3 * i + 1] - (double)R[1],
               dz = (double)r[3 * i + 2] - (double)R[2];
  const double radius = sqrt(dx * dx + dy * dy + dz * dz);
  double ct = dz / radius;                                   // ecp_utils.py:53 (clip to [-1, 1])
  ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
  const double st = sqrt(1.0 - ct * ct);                     // sin(arccos(.)) >= 0
  const double phi = atan2(dy, dx);
  double phr;
  const long bg = a.walker_idx ? (long)a.walker_idx[b] : (long)b;          // index that keys the rotation angle
  if (a.phi != nullptr) {
    const long pidx = (bg * a.n_nl + j) * N + i;
    phr = a.phi_f32 ? (double)reinterpret_cast<const float*>(a.phi)[pidx] : (double)reinterpret_cast<const real*>(a.phi)[pidx];
  } else {
    uint32_t o[4];
    philox4x32(a.seed, 0x45435000ull + (uint64_t)j, (uint64_t)bg * (uint64_t)N + (uint64_t)i, o);
    phr = u01(o[0], o[1]) * 0.62831853071795865;             // U[0, pi/5), ecp_utils.py:55
  }
  // u = rot_z(phr) * unit vertex; v = rot_y(theta) u; w = rot_z(phi) v
  const double cq = ico_cos(q), sq = sqrt(1.0 - cq * cq), pq = ico_phi(q) + phr;
  const double ux = sq * cos(pq), uy = sq * sin(pq), uz = cq;
  const double vx = ct * ux + st * uz, vy = uy, vz = -st * ux + ct * uz;
  const double cp = cos(phi), sp = sin(phi);
  const double w[3] = {cp * vx - sp * vy, sp * vx + cp * vy, vz};
  rq[idx] = (real)(radius * w[c] + (double)R[c]);
}

// One thread per walker of the chunk: V_nl from the psi ratios; added to e_loc and stored in stats[3].
template <typename real>
__global__ void __launch_bounds__(64) k_ecp_reduce(const EcpArgs a, const real* __restrict__ logq,
                                                   const int32_t* __restrict__ signq, const real* __restrict__ log0,
                                                   const int32_t* __restrict__ sign0, real* __restrict__ e_loc,
                                                   real* __restrict__ stats, real* __restrict__ v_nl_out) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= a.nb) return;
  const int b = a.b0 + bl, N = a.N;
  const real* r = reinterpret_cast<const real*>(a.r) + (long)b * N * 3;
  const double l0 = (double)log0[b];
  const int s0 = sign0[b];
  double total = 0.0;
  for (int j = 0; j < a.n_nl; ++j) {
    const real* R = reinterpret_cast<const real*>(a.R) + 3 * a.nl_nuc[j];
    const double* nl = a.nl + (long)j * a.L * 2 * a.n_t;
    for (int i = 0; i < N; ++i) {
      double d2 = 0.0;
      for (int c = 0; c < 3; ++c) { const double d = (double)r[3 * i + c] - (double)R[c]; d2 += d * d; }
      const long base = (((long)bl * a.n_nl + j) * N + i) * 12;
      double ratio[12];
      for (int q = 0; q < 12; ++q)
        ratio[q] = exp((double)logq[base + q] - l0) * (double)(signq[base + q] * s0);   // ecp_utils.py:92-95
      for (int l = 0; l < a.L; ++l) {
        double vl = 0.0;                                                               // V_l(r), :207-211
        for (int t = 0; t < a.n_t; ++t) vl += nl[(l * 2 + 1) * a.n_t + t] * exp(-d2 * nl[(l * 2) * a.n_t + t]);
        if (vl == 0.0) continue;
        double integral = 0.0;
        for (int q = 0; q < 12; ++q) {
          const double x = ico_cos(q);
          double pm = 1.0, p = x;                     // Legendre recurrence
          double pl = l == 0 ? 1.0 : x;
          for (int m = 2; m <= l; ++m) { pl = ((2 * m - 1) * x * p - (m - 1) * pm) / m; pm = p; p = pl; }
          integral += ratio[q] * pl;
        }
        total += vl * (2 * l + 1) / 12.0 * integral;
      }
    }
  }
  if (e_loc) e_loc[b] = (real)((double)e_loc[b] + total);
  if (stats) stats[3L * a.B + b] = (real)total;
  if (v_nl_out) v_nl_out[b] = (real)total;
}

// ---- mixed-precision quadrature of a float32 context (engine.hip: ecp_mixed) ------------------------------------------------
// The float32 value path puts ~1e-4 on log|psi| of a 30-electron Psiformer, i.e. on every psi ratio; V_nl is a sum of
// 12 N n_ecp of them weighted by (2l+1)/12 V_l(|r_i - R_a|), and V_l is a Gaussian of the electron-nucleus distance: a
// few electron-nucleus pairs carry the sum.  Every (walker, ECP nucleus a, electron i) triple is classified by
//     w = max_l (2l+1) |V_l(|r_i - R_a|)|      (the bound of its contribution per unit of its quadrature mean)
//   w >  w_heavy : its 12 psi ratios are evaluated by the float64 twin (numerator AND denominator in float64),
//   w <= w_skip  : dropped -- its contribution is below w_skip |mean ratio|, ~1e-10 Ha,
//   otherwise    : float32, with psi(r) of the walker evaluated through the SAME float32 value path as the 12 moved
//                  configurations (the errors of numerator and denominator are those of one arithmetic).
// The class depends on the walker's geometry alone.  Classified triples are compacted with an atomic counter: list ORDER
// varies from call to call, results do not (every configuration is evaluated independently and stored at its own slot).
constexpr int32_t ECP_SKIP = INT32_MIN;
__device__ __forceinline__ void ecp_vertex(const double ri[3], const double Rn[3], double phr, int q, double out[3]) {
  const double dx = ri[0] - Rn[0], dy = ri[1] - Rn[1], dz = ri[2] - Rn[2];
  const double radius = sqrt(dx * dx + dy * dy + dz * dz);
  double ct = dz / radius;                                   // ecp_utils.py:53 (clip to [-1, 1])
  ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
  const double st = sqrt(1.0 - ct * ct);
  const double phi = atan2(dy, dx);
  const double cq = ico_cos(q), sq = sqrt(1.0 - cq * cq), pq = ico_phi(q) + phr;
  const double ux = sq * cos(pq), uy = sq * sin(pq), uz = cq;
  const double vx = ct * ux + st * uz, vy = uy, vz = -st * ux + ct * uz;
  const double cp = cos(phi), sp = sin(phi);
  out[0] = radius * (cp * vx - sp * vy) + Rn[0];
  out[1] = radius * (sp * vx + cp * vy) + Rn[1];
  out[2] = radius * vz + Rn[2];
}
__device__ __forceinline__ double ecp_angle(const EcpMixArgs& a, int b, int j, int i) {
  if (a.phi != nullptr) return (double)a.phi[((long)b * a.n_nl + j) * a.N + i];
  uint32_t o[4];
  philox4x32(a.seed, 0x45435000ull + (uint64_t)j, (uint64_t)b * (uint64_t)a.N + (uint64_t)i, o);
  return u01(o[0], o[1]) * 0.62831853071795865;             // U[0, pi/5), ecp_utils.py:55
}
// one thread per triple t = (bl * n_nl + j) * N + i of the chunk
__global__ void __launch_bounds__(256) k_ecp_classify(const EcpMixArgs a, int32_t* __restrict__ cls, int32_t* __restrict__ list_l,
                                                      int32_t* __restrict__ list_h, int32_t* __restrict__ counts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nb * a.n_nl * a.N) return;
  const int i = t % a.N, j = (t / a.N) % a.n_nl, bl = t / (a.N * a.n_nl);
  const float* r = a.r + ((long)(a.b0 + bl) * a.N + i) * 3;
  const float* R = a.R + 3 * a.nl_nuc[j];
  double d2 = 0.0;
  for (int c = 0; c < 3; ++c) { const double d = (double)r[c] - (double)R[c]; d2 += d * d; }
  const double* nl = a.nl + (long)j * a.L * 2 * a.n_t;
  double w = 0.0;
  for (int l = 0; l < a.L; ++l) {
    double vl = 0.0;
    for (int k = 0; k < a.n_t; ++k) vl += nl[(l * 2 + 1) * a.n_t + k] * exp(-d2 * nl[(l * 2) * a.n_t + k]);
    w = fmax(w, (2 * l + 1) * fabs(vl));
  }
  if (!(w > a.w_skip)) { cls[t] = ECP_SKIP; return; }
  double amp = 1.0;            // how much worse than ordinary float32 this walker's psi(r) is (EcpMixArgs::l32)
  if (a.l32 != nullptr) {
    const double dl = fabs((double)a.l32[bl] - a.l64[bl]);
    amp = (a.s32[bl] != a.s64[bl] || !(dl == dl)) ? HUGE_VAL : fmax(1.0, dl / a.dlog_floor);
  }
  if (w * amp > a.w_heavy) { const int pos = atomicAdd(&counts[1], 1); list_h[pos] = t; cls[t] = -(pos + 1); }
  else { const int pos = atomicAdd(&counts[0], 1); list_l[pos] = t; cls[t] = pos; }
}
// configurations of one class: [0, nb) the walkers of the chunk themselves, then 12 per listed triple.  One thread per coordinate.
template <typename real_out>
__global__ void __launch_bounds__(256) k_ecp_points_list(const EcpMixArgs a, const int32_t* __restrict__ list, int n_list,
                                                         real_out* __restrict__ rq) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.N;
  const long per_cfg = (long)N * 3;
  const long n_cfg = (long)a.nb + 12L * n_list;
  if (idx >= n_cfg * per_cfg) return;
  const long cfg = idx / per_cfg;
  const int ec = (int)(idx - cfg * per_cfg), e = ec / 3, c = ec - 3 * e;
  if (cfg < a.nb) { rq[idx] = (real_out)a.r[(long)(a.b0 + cfg) * per_cfg + ec]; return; }
  const long k = cfg - a.nb;
  const int t = list[k / 12], q = (int)(k % 12);
  const int i = t % N, j = (t / N) % a.n_nl, bl = t / (N * a.n_nl);
  const int b = a.b0 + bl;
  const float* r = a.r + (long)b * per_cfg;
  if (e != i) { rq[idx] = (real_out)r[ec]; return; }
  const float* R = a.R + 3 * a.nl_nuc[j];
  const double ri[3] = {(double)r[3 * i], (double)r[3 * i + 1], (double)r[3 * i + 2]};
  const double Rn[3] = {(double)R[0], (double)R[1], (double)R[2]};
  double x[3];
  ecp_vertex(ri, Rn, ecp_angle(a, b, j, i), q, x);
  rq[idx] = (real_out)x[c];
}
// one thread per walker of the chunk: V_nl from the ratios of both classes; added to e_loc, stored in stats[3]
__global__ void __launch_bounds__(64) k_ecp_reduce_mixed(const EcpMixArgs a, const int32_t* __restrict__ cls,
                                                         const float* __restrict__ lq32, const int32_t* __restrict__ sq32,
                                                         const double* __restrict__ lq64, const int32_t* __restrict__ sq64,
                                                         float* __restrict__ e_loc, float* __restrict__ stats) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= a.nb) return;
  const int b = a.b0 + bl, N = a.N;
  const float* r = a.r + (long)b * N * 3;
  const double l0_32 = (double)lq32[bl], l0_64 = lq64[bl];
  const int s0_32 = sq32[bl], s0_64 = sq64[bl];
  double total = 0.0;
  for (int j = 0; j < a.n_nl; ++j) {
    const float* R = a.R + 3 * a.nl_nuc[j];
    const double* nl = a.nl + (long)j * a.L * 2 * a.n_t;
    for (int i = 0; i < N; ++i) {
      const int32_t c = cls[((long)bl * a.n_nl + j) * N + i];
      if (c == ECP_SKIP) continue;
      double d2 = 0.0;
      for (int x = 0; x < 3; ++x) { const double d = (double)r[3 * i + x] - (double)R[x]; d2 += d * d; }
      double ratio[12];
      if (c >= 0) {
        const long base = (long)a.nb + 12L * c;
        for (int q = 0; q < 12; ++q) ratio[q] = exp((double)lq32[base + q] - l0_32) * (double)(sq32[base + q] * s0_32);
      } else {
        const long base = (long)a.nb + 12L * (-(long)c - 1);
        for (int q = 0; q < 12; ++q) ratio[q] = exp(lq64[base + q] - l0_64) * (double)(sq64[base + q] * s0_64);
      }
      for (int l = 0; l < a.L; ++l) {
        double vl = 0.0;
        for (int t = 0; t < a.n_t; ++t) vl += nl[(l * 2 + 1) * a.n_t + t] * exp(-d2 * nl[(l * 2) * a.n_t + t]);
        if (vl == 0.0) continue;
        double integral = 0.0;
        for (int q = 0; q < 12; ++q) {
          const double x = ico_cos(q);
          double pm = 1.0, p = x;
          double pl = l == 0 ? 1.0 : x;
          for (int m = 2; m <= l; ++m) { pl = ((2 * m - 1) * x * p - (m - 1) * pm) / m; pm = p; p = pl; }
          integral += ratio[q] * pl;
        }
        total += vl * (2 * l + 1) / 12.0 * integral;
      }
    }
  }
  if (e_loc) e_loc[b] = (float)((double)e_loc[b] + total);
  if (stats) stats[3L * a.B + b] = (float)total;
}
void launch_ecp_classify(hipStream_t st, const EcpMixArgs& a, int32_t* cls, int32_t* list_l, int32_t* list_h, int32_t* counts) {
  const long n = (long)a.nb * a.n_nl * a.N;
  hipLaunchKernelGGL(k_ecp_classify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, cls, list_l, list_h, counts);
}
template <typename real_out> void launch_ecp_points_list(hipStream_t st, const EcpMixArgs& a, const int32_t* list, int n_list, real_out* rq) {
  const long n = ((long)a.nb + 12L * n_list) * a.N * 3;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_points_list<real_out>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, list, n_list, rq);
}
template void launch_ecp_points_list<float>(hipStream_t, const EcpMixArgs&, const int32_t*, int, float*);
template void launch_ecp_points_list<double>(hipStream_t, const EcpMixArgs&, const int32_t*, int, double*);
void launch_ecp_reduce_mixed(hipStream_t st, const EcpMixArgs& a, const int32_t* cls, const float* lq32, const int32_t* sq32,
                             const double* lq64, const int32_t* sq64, float* e_loc, float* stats) {
  hipLaunchKernelGGL(k_ecp_reduce_mixed, dim3((unsigned)((a.nb + 63) / 64)), dim3(64), 0, st, a, cls, lq32, sq32, lq64, sq64, e_loc, stats);
}

template <typename real> void launch_ecp_points(hipStream_t st, const EcpArgs& a, real* rq) {
  const long n = (long)a.nb * a.n_nl * a.N * 12 * a.N * 3;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_points<real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, rq);
}
template <typename real>
void launch_ecp_reduce(hipStream_t st, const EcpArgs& a, const real* logq, const int32_t* signq, const real* log0,
                       const int32_t* sign0, real* e_loc, real* stats, real* v_nl_out) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_reduce<real>), dim3((unsigned)((a.nb + 63) / 64)), dim3(64), 0, st, a, logq,
                     signq, log0, sign0, e_loc, stats, v_nl_out);
}

// ---- Hellmann-Feynman force of a Gaussian-type ECP Hamiltonian (dqmc_ecp_force; engine_ecp_force.inl) ------------------------
// Reference: force.py:286-299 (evaluate_hf_force_bare with hamil.pot.grad_nonloc_potential), ecp/gaussian_type_ecp.py:257-330,
// ecp/ecp_force_utils.py.  Per walker, F_I = F_nuc,I(Z) - dV_loc/dR_I - G_I with G the gradient of the non-local term.  For the
// nucleus I = nl_nuc[j], electron i and vertex q (x_q = R_I + rho w_q, d = r_i - R_I, rho = |d|, ecp_vertex above):
//   ratio_q        = s_q s_0 exp(log_q - log_0)
//   dratio_q/dR_K  = ratio_q (gR_q[K] - gR_0[K] + [K == I] J_q^T gr_q[i]),     J_q = dx_q/dR_I (ecp_vertex_jt below)
//   G_K           += sum_i sum_l (2l+1)/12 [ [K == I] dv_l/dR_I sum_q P_l(cos theta_q) ratio_q + v_l sum_q P_l(cos theta_q) dratio_q/dR_K ]
// with gr_q / gR_q = d log|psi| / dr, / dR at the configuration with electron i at x_q (the Coords reverse pass) and gR_0 the
// same at the walker itself.  Vertex 0 is the electron itself whatever R is (ratio 1, derivative 0): it is not part of the
// batch (11 configurations per triple) and enters the dv_l term with ratio 1.  The sums over l are taken first:
//   c_q = sum_l (2l+1)/12 v_l P_l(cos theta_q),   e_q = sum_l (2l+1)/12 (sum_t alpha_lt beta_lt e^{-alpha_lt rho^2}) P_l(cos theta_q)
//   G_K = sum_i [ sum_q c_q ratio_q (gR_q[K] - gR_0[K]) ] + [K == I] sum_i [ sum_q ratio_q (2 d e_q + c_q J_q^T gr_q[i]) ].

template <typename real>
__device__ __forceinline__ double ecp_angle_of(const EcpArgs& a, int b, int j, int i) {       // the angle k_ecp_points uses
  const long bg = a.walker_idx ? (long)a.walker_idx[b] : (long)b;
  if (a.phi != nullptr) {
    const long pidx = (bg * a.n_nl + j) * a.N + i;
    return a.phi_f32 ? (double)reinterpret_cast<const float*>(a.phi)[pidx] : (double)reinterpret_cast<const real*>(a.phi)[pidx];
  }
  uint32_t o[4];
  philox4x32(a.seed, 0x45435000ull + (uint64_t)j, (uint64_t)bg * (uint64_t)a.N + (uint64_t)i, o);
  return u01(o[0], o[1]) * 0.62831853071795865;
}

// J_q^T g for vertex q of ecp_vertex: x_q = R + rho w(theta, phi), theta = arccos(d_z / rho), phi = atan2(d_y, d_x), so
//   J_q = dx_q/dR = 1 - [ w dhat^T + rho (d_theta w)(grad_d theta)^T + rho (d_phi w)(grad_d phi)^T ],
//   grad_d theta = (cos(theta) dhat - e_z) / (rho sin(theta)),   grad_d phi = (-d_y, d_x, 0) / (d_x^2 + d_y^2).
// The same frame (ct, st, phi, u, v) as ecp_vertex; singular on the axis d || e_z, as the reference's autograd is.
__device__ __forceinline__ void ecp_vertex_jt(const double d[3], double phr, int q, const double g[3], double out[3]) {
  const double dx = d[0], dy = d[1], dz = d[2];
  const double radius = sqrt(dx * dx + dy * dy + dz * dz);
  double ct = dz / radius;
  ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
  const double st = sqrt(1.0 - ct * ct);
  const double phi = atan2(dy, dx);
  const double cq = ico_cos(q), sq = sqrt(1.0 - cq * cq), pq = ico_phi(q) + phr;
  const double ux = sq * cos(pq), uy = sq * sin(pq), uz = cq;
  const double vx = ct * ux + st * uz, vy = uy, vz = -st * ux + ct * uz;
  const double tx = -st * ux + ct * uz, tz = -ct * ux - st * uz;          // d_theta v (its y component is 0)
  const double cp = cos(phi), sp = sin(phi);
  const double wg = (cp * vx - sp * vy) * g[0] + (sp * vx + cp * vy) * g[1] + vz * g[2];        // w . g
  const double tg = cp * tx * g[0] + sp * tx * g[1] + tz * g[2];                                // d_theta w . g
  const double pg = (-sp * vx - cp * vy) * g[0] + (cp * vx - sp * vy) * g[1];                   // d_phi w . g
  const double hx = dx / radius, hy = dy / radius, hz = dz / radius;
  const double it = tg / st, ip = pg * radius / (dx * dx + dy * dy);
  out[0] = g[0] - hx * wg - (ct * hx) * it + dy * ip;
  out[1] = g[1] - hy * wg - (ct * hy) * it - dx * ip;
  out[2] = g[2] - hz * wg - (ct * hz - 1.0) * it;
}

// Configurations of the chunk [b0, b0 + nb): [0, nb) the walkers themselves, then ECPF_NQ per triple t = (bl n_nl + j) N + i:
// configuration nb + t ECPF_NQ + (q - 1) is walker b0 + bl with electron i at vertex q.  One thread per coordinate.
template <typename real>
__global__ void __launch_bounds__(256) k_ecp_force_points(const EcpArgs a, real* __restrict__ rq) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.N;
  const long per_cfg = (long)N * 3;
  const long n_cfg = (long)a.nb + (long)ECPF_NQ * a.nb * a.n_nl * N;
  if (idx >= n_cfg * per_cfg) return;
  const long cfg = idx / per_cfg;
  const int ec = (int)(idx - cfg * per_cfg), e = ec / 3, c = ec - 3 * e;
  const real* rall = reinterpret_cast<const real*>(a.r);
  if (cfg < a.nb) { rq[idx] = rall[(long)(a.b0 + cfg) * per_cfg + ec]; return; }
  const long k = cfg - a.nb;
  const long t = k / ECPF_NQ;
  const int q = 1 + (int)(k - t * ECPF_NQ);
  const int i = (int)(t % N), j = (int)((t / N) % a.n_nl), bl = (int)(t / ((long)N * a.n_nl));
  const int b = a.b0 + bl;
  const real* r = rall + (long)b * per_cfg;
  if (e != i) { rq[idx] = r[ec]; return; }
  const real* R = reinterpret_cast<const real*>(a.R) + 3 * a.nl_nuc[j];
  const double ri[3] = {(double)r[3 * i], (double)r[3 * i + 1], (double)r[3 * i + 2]};
  const double Rn[3] = {(double)R[0], (double)R[1], (double)R[2]};
  double x[3];
  ecp_vertex(ri, Rn, ecp_angle_of<real>(a, b, j, i), q, x);
  rq[idx] = (real)x[c];
}

__device__ __forceinline__ double ecpf_grp16_sum(double v) {      // fixed tree over the 16 lanes of a group
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One wave per (walker bl of the chunk, non-local nucleus j): gj[bl][j][K][3] = that nucleus's contribution to G_K, double.
// Lane = (group g = lane / 16, vertex q = lane % 16; q >= 12 idle): group g takes the electrons g, g + 4, ...  Per electron
// the vertices are summed by the xor tree of the group; the electrons are then summed in index order.  No atomics.
// all_rows == 0: only the row K == I = nl_nuc[j] is formed, the others are zero.
template <typename real>
__global__ void __launch_bounds__(64) k_ecp_force_reduce(const EcpArgs a, int n_nuc, int all_rows, const real* __restrict__ lq,
                                                         const int32_t* __restrict__ sq, const real* __restrict__ gr,
                                                         const real* __restrict__ gR, double* __restrict__ gj) {
  __shared__ double s_w[GRAD_GJ_NMAX][16];       // c_q ratio_q of (electron, vertex); 0 for q = 0 and the idle lanes
  __shared__ double s_own[GRAD_GJ_NMAX][3];      // sum_q ratio_q (2 d e_q + c_q J_q^T gr_q[i]) per electron
  __shared__ double s_part[GRAD_GJ_NMAX][3];     // sum_q c_q ratio_q (gR_q[K] - gR_0[K]) per electron, for the current K
  const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
  const int N = a.N, n_nl = a.n_nl;
  const int bl = blockIdx.x / n_nl, j = blockIdx.x - bl * n_nl;
  const int b = a.b0 + bl, I = a.nl_nuc[j];
  const real* r = reinterpret_cast<const real*>(a.r) + (long)b * N * 3;
  const real* R = reinterpret_cast<const real*>(a.R) + 3 * I;
  const double* nl = a.nl + (long)j * a.L * 2 * a.n_t;
  const double l0 = (double)lq[bl];
  const int s0 = sq[bl];
  const long cfg0 = (long)a.nb + ((long)bl * n_nl + j) * N * ECPF_NQ;      // first configuration of the pair's triples
  for (int i0 = 0; i0 < N; i0 += 4) {
    const int i = i0 + g;
    double own0 = 0.0, own1 = 0.0, own2 = 0.0, w = 0.0;
    if (i < N && q < 12) {
      const double d[3] = {(double)r[3 * i] - (double)R[0], (double)r[3 * i + 1] - (double)R[1], (double)r[3 * i + 2] - (double)R[2]};
      const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      const double x = ico_cos(q);
      double cq = 0.0, eq = 0.0, pm = 1.0, p = x;
      for (int l = 0; l < a.L; ++l) {
        double pl = l == 0 ? 1.0 : x;                 // Legendre recurrence, as k_ecp_reduce
        if (l >= 2) { pl = ((2 * l - 1) * x * p - (l - 1) * pm) / l; pm = p; p = pl; }
        double vl = 0.0, al = 0.0;
        for (int t = 0; t < a.n_t; ++t) {
          const double alpha = nl[(l * 2) * a.n_t + t], term = nl[(l * 2 + 1) * a.n_t + t] * exp(-d2 * alpha);
          vl += term; al += alpha * term;
        }
        cq += (2 * l + 1) / 12.0 * vl * pl;
        eq += (2 * l + 1) / 12.0 * al * pl;
      }
      double ratio = 1.0, jt[3] = {0.0, 0.0, 0.0};
      if (q > 0) {
        const long cfg = cfg0 + (long)i * ECPF_NQ + (q - 1);
        const double lg = (double)lq[cfg];
        const int s = sq[cfg];
        ratio = (s != 0 && lg - lg == 0) ? exp(lg - l0) * (double)(s * s0) : 0.0;      // an invalid numerator: ratio 0
        const real* gq = gr + (cfg * N + i) * 3;
        const double gv[3] = {(double)gq[0], (double)gq[1], (double)gq[2]};
        ecp_vertex_jt(d, ecp_angle_of<real>(a, b, j, i), q, gv, jt);
        w = cq * ratio;
      }
      own0 = ratio * (2.0 * d[0] * eq) + w * jt[0];
      own1 = ratio * (2.0 * d[1] * eq) + w * jt[1];
      own2 = ratio * (2.0 * d[2] * eq) + w * jt[2];
    }
    own0 = ecpf_grp16_sum(own0); own1 = ecpf_grp16_sum(own1); own2 = ecpf_grp16_sum(own2);
    if (i < N) {
      s_w[i][q] = w;
      if (q == 0) { s_own[i][0] = own0; s_own[i][1] = own1; s_own[i][2] = own2; }
    }
  }
  __syncthreads();
  double* out = gj + (long)blockIdx.x * n_nuc * 3;
  for (int K = 0; K < n_nuc; ++K) {
    if (!all_rows && K != I) {
      if (lane < 3) out[K * 3 + lane] = 0.0;
      continue;
    }
    const real* g0 = gR + ((long)bl * n_nuc + K) * 3;
    for (int i0 = 0; i0 < N; i0 += 4) {
      const int i = i0 + g;
      double v0 = 0.0, v1 = 0.0, v2 = 0.0;
      if (i < N && q > 0 && q < 12) {
        const double w = s_w[i][q];
        const real* gq = gR + ((cfg0 + (long)i * ECPF_NQ + (q - 1)) * n_nuc + K) * 3;
        v0 = w * ((double)gq[0] - (double)g0[0]);
        v1 = w * ((double)gq[1] - (double)g0[1]);
        v2 = w * ((double)gq[2] - (double)g0[2]);
      }
      v0 = ecpf_grp16_sum(v0); v1 = ecpf_grp16_sum(v1); v2 = ecpf_grp16_sum(v2);
      if (i < N && q == 0) { s_part[i][0] = v0; s_part[i][1] = v1; s_part[i][2] = v2; }
    }
    __syncthreads();
    if (lane < 3) {
      double s = 0.0;
      for (int i = 0; i < N; ++i) s += s_part[i][lane];
      if (K == I) {
        double o = 0.0;
        for (int i = 0; i < N; ++i) o += s_own[i][lane];
        s += o;
      }
      out[K * 3 + lane] = s;
    }
    __syncthreads();
  }
}

// One thread per (walker bl of the chunk, nucleus K): F_nuc(Z) - dV_loc/dR_K (nuclear repulsion of the valence charges, the
// -Z/rho attraction and the local ECP terms of gaussian_type_ecp.py:127-159: with f_K the radial function of nucleus K,
// dV_loc/dR_K = -sum_i f_K'(rho) d / rho), minus G_K summed over the non-local nuclei in index order, and the optional
// zero-bias term -2 (e_loc - energy) gR_0[K].  lq / sq / gR: the walkers' own log|psi|, sign and d log|psi| / dR where a
// reverse pass has run (else nullptr); a walker with sign 0 or a non-finite log|psi| gets NaN rows in force and parts[1].
template <typename real>
__global__ void __launch_bounds__(256) k_ecp_force_local(const EcpArgs a, int n_nuc, const double* __restrict__ Z,
                                                         const double* __restrict__ loc, int nt_loc, const double* __restrict__ gj,
                                                         const real* __restrict__ lq, const int32_t* __restrict__ sq,
                                                         const real* __restrict__ gR, const real* __restrict__ e_loc, double energy,
                                                         double* __restrict__ force, double* __restrict__ part0,
                                                         double* __restrict__ part1) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)a.nb * n_nuc) return;
  const int K = (int)(idx % n_nuc), bl = (int)(idx / n_nuc), N = a.N;
  const long b = a.b0 + bl;
  const real* r = reinterpret_cast<const real*>(a.r) + b * N * 3;
  const real* R = reinterpret_cast<const real*>(a.R);
  double f[3] = {0, 0, 0};
  for (int J = 0; J < n_nuc; ++J) {           // nuclear repulsion, as k_hf_force
    if (J == K) continue;
    double d[3], d2 = 0;
    for (int c = 0; c < 3; ++c) { d[c] = (double)R[K * 3 + c] - (double)R[J * 3 + c]; d2 += d[c] * d[c]; }
    const double w = Z[K] * Z[J] / (d2 * sqrt(d2));
    for (int c = 0; c < 3; ++c) f[c] += w * d[c];
  }
  const double* p = loc ? loc + (long)K * 6 * nt_loc : nullptr;
  double fe[3] = {0, 0, 0};
  for (int i = 0; i < N; ++i) {
    double d[3], d2 = 0;
    for (int c = 0; c < 3; ++c) { d[c] = (double)r[i * 3 + c] - (double)R[K * 3 + c]; d2 += d[c] * d[c]; }
    const double rho = sqrt(d2);
    double fp = Z[K] / d2;                     // f'(rho) of -Z / rho
    if (p)
      for (int t = 0; t < nt_loc; ++t) {       // beta/rho e^{-alpha rho^2}, beta e^{-alpha rho^2}, beta rho e^{-alpha rho^2}
        fp -= p[1 * nt_loc + t] * exp(-p[0 * nt_loc + t] * d2) * (1.0 / d2 + 2.0 * p[0 * nt_loc + t]);
        fp -= p[3 * nt_loc + t] * exp(-p[2 * nt_loc + t] * d2) * (2.0 * p[2 * nt_loc + t] * rho);
        fp += p[5 * nt_loc + t] * exp(-p[4 * nt_loc + t] * d2) * (1.0 - 2.0 * p[4 * nt_loc + t] * d2);
      }
    for (int c = 0; c < 3; ++c) fe[c] += fp * d[c] / rho;
  }
  const bool valid = !lq || (sq[bl] != 0 && (double)lq[bl] - (double)lq[bl] == 0);
  const double de = e_loc ? -2.0 * ((double)e_loc[b] - energy) : 0.0;
  for (int c = 0; c < 3; ++c) {
    const double p0 = f[c] + fe[c];
    double p1 = 0.0;
    if (gj) {
      double s = 0.0;
      for (int j = 0; j < a.n_nl; ++j) s += gj[(((long)bl * a.n_nl + j) * n_nuc + K) * 3 + c];
      p1 = valid ? 0.0 - s : NAN;
    }
    double tot = p0 + p1;
    if (e_loc) tot += de * (double)gR[((long)bl * n_nuc + K) * 3 + c];
    if (!valid) tot = NAN;
    force[(b * n_nuc + K) * 3 + c] = tot;
    if (part0) { part0[(b * n_nuc + K) * 3 + c] = p0; part1[(b * n_nuc + K) * 3 + c] = p1; }
  }
}

template <typename real> void launch_ecp_force_points(hipStream_t st, const EcpArgs& a, real* rq) {
  const long n = ((long)a.nb + (long)ECPF_NQ * a.nb * a.n_nl * a.N) * a.N * 3;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_force_points<real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, rq);
}
template <typename real>
void launch_ecp_force_reduce(hipStream_t st, const EcpArgs& a, int n_nuc, int all_rows, const real* lq, const int32_t* sq, const real* gr,
                             const real* gR, double* gj) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_force_reduce<real>), dim3((unsigned)(a.nb * a.n_nl)), dim3(64), 0, st, a, n_nuc, all_rows, lq, sq,
                     gr, gR, gj);
}
template <typename real>
void launch_ecp_force_local(hipStream_t st, const EcpArgs& a, int n_nuc, const double* Z, const double* loc, int nt_loc, const double* gj,
                            const real* lq, const int32_t* sq, const real* gR, const real* e_loc, double energy, double* force,
                            double* part0, double* part1) {
  const long n = (long)a.nb * n_nuc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ecp_force_local<real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, n_nuc, Z, loc, nt_loc,
                     gj, lq, sq, gR, e_loc, energy, force, part0, part1);
}

// ---- pseudo-Hamiltonian coefficients ----------------------------------------------------------------------------
// Reference: ecp/pseudo_hamiltonian.py:173-234.  For electron i of walker b, with d_I = r_i - R_I, rho_I = |d_I|
// (plain norm, geom/general.py:19-21) and the tabulated radial functions rV_loc / rV_L2 of the PH nuclei (linear
// interpolation on the regular grid [0, r_max], zero outside -- RegularGridInterpolator(fill_value=0), :95-101):
//   A_i = 1/2 I + sum_I [ rV_L2(rho) rho I - rV_L2(rho)/rho d d^T ],    b_i = sum_I 2 rV_L2(rho)/rho d,
//   V_ph(b) = sum_i sum_I rV_loc(rho)/rho.
// Written per (walker, electron): the lower Cholesky factor Q of A (jax.scipy.linalg.cholesky(A, lower=True), :257)
// Q^-1 b (so that b . grad_r = (Q^-1 b) . grad_v, :268-271) and the electron's share of V_ph (k_final sums them).
__device__ __forceinline__ double ph_interp(const double* tab, int n_grid, double inv_h, double rho) {
  const double x = rho * inv_h;
  if (!(x >= 0.0) || x > (double)(n_grid - 1)) return 0.0;
  int k = (int)x;
  if (k > n_grid - 2) k = n_grid - 2;
  const double f = x - k;
  return tab[k] + f * (tab[k + 1] - tab[k]);
}
template <typename real>
__global__ void __launch_bounds__(256) k_ph_coeffs(const real* __restrict__ r, const real* __restrict__ R,
                                                   const int32_t* __restrict__ ph_nuc, int n_ph,
                                                   const double* __restrict__ rv_loc, const double* __restrict__ rv_l2,
                                                   int n_grid, double r_max, int B, int N, double* __restrict__ phq) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * N) return;
  const double inv_h = (double)(n_grid - 1) / r_max;
  const real* ri = r + (long)idx * 3;
  double A[3][3] = {{0.5, 0, 0}, {0, 0.5, 0}, {0, 0, 0.5}}, bv[3] = {0, 0, 0}, vloc = 0.0;
  for (int j = 0; j < n_ph; ++j) {
    const real* Rn = R + ph_nuc[j] * 3;
    double d[3], d2 = 0.0;
    for (int c = 0; c < 3; ++c) { d[c] = (double)ri[c] - (double)Rn[c]; d2 += d[c] * d[c]; }
    const double rho = sqrt(d2);
    const double rvl2 = ph_interp(rv_l2 + (long)j * n_grid, n_grid, inv_h, rho);
    const double v = rvl2 / rho;
    vloc += ph_interp(rv_loc + (long)j * n_grid, n_grid, inv_h, rho) / rho;
    for (int a = 0; a < 3; ++a) {
      bv[a] += 2.0 * v * d[a];
      A[a][a] += rvl2 * rho;
      for (int c = 0; c < 3; ++c) A[a][c] -= v * d[a] * d[c];
    }
  }
  // lower Cholesky factor (a non-positive pivot gives NaN, as LAPACK potrf does through jax)
  double Q[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  Q[0][0] = sqrt(A[0][0]);
  Q[1][0] = A[1][0] / Q[0][0];
  Q[2][0] = A[2][0] / Q[0][0];
  Q[1][1] = sqrt(A[1][1] - Q[1][0] * Q[1][0]);
  Q[2][1] = (A[2][1] - Q[2][0] * Q[1][0]) / Q[1][1];
  Q[2][2] = sqrt(A[2][2] - Q[2][0] * Q[2][0] - Q[2][1] * Q[2][1]);
  double y[3];
  y[0] = bv[0] / Q[0][0];
  y[1] = (bv[1] - Q[1][0] * y[0]) / Q[1][1];
  y[2] = (bv[2] - Q[2][0] * y[0] - Q[2][1] * y[1]) / Q[2][2];
  double* o = phq + (long)idx * PH_STRIDE;
  for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) o[3 * a + c] = Q[a][c];
  for (int a = 0; a < 3; ++a) o[9 + a] = y[a];
  o[12] = vloc;
}
template <typename real>
void launch_ph_coeffs(hipStream_t st, const real* r, const real* R, const int32_t* ph_nuc, int n_ph, const double* rv_loc,
                      const double* rv_l2, int n_grid, double r_max, int B, int N, double* phq) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ph_coeffs<real>), dim3((unsigned)(((long)B * N + 255) / 256)), dim3(256), 0, st, r, R,
                     ph_nuc, n_ph, rv_loc, rv_l2, n_grid, r_max, B, N, phq);
}

#define DQMC_INST(real)                                                                                            \
  template void launch_ph_coeffs<real>(hipStream_t, const real*, const real*, const int32_t*, int, const double*,  \
                                       const double*, int, double, int, int, double*);                             \
  template void launch_ecp_points<real>(hipStream_t, const EcpArgs&, real*);                                       \
  template void launch_ecp_reduce<real>(hipStream_t, const EcpArgs&, const real*, const int32_t*, const real*,     \
                                        const int32_t*, real*, real*, real*);                                      \
  template void launch_ecp_force_points<real>(hipStream_t, const EcpArgs&, real*);                                 \
  template void launch_ecp_force_reduce<real>(hipStream_t, const EcpArgs&, int, int, const real*, const int32_t*,  \
                                              const real*, const real*, double*);                                  \
  template void launch_ecp_force_local<real>(hipStream_t, const EcpArgs&, int, const double*, const double*, int,  \
                                             const double*, const real*, const int32_t*, const real*, const real*, \
                                             double, double*, double*, double*);
DQMC_INST(float)
DQMC_INST(double)
#undef DQMC_INST

}  // namespace dqmc

#include "kernels_observable.inl"
