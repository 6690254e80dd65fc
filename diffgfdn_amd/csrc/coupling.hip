// Coupled feedback matrices of all bands of a band bank on the device, for gfx950.
//
// reference: feedback_loop.py:39-87 (ND_Unitary: Phi from G(G-1)/2 Givens angles), :393-404 (block (i,j) of the mixing
// matrix = Q_i Q_j), :406-455 (SCALAR coupling: A = block_M o kron(Phi, 1), angles clamped to [-pi, pi]; G = 1: block_M).
//   forward : Phi = U_G,  U_m = (R_{m-2} .. R_0) diag(U_{m-1}, 1),  A[(i,a),(j,c)] = Phi_ij sum_b Q_i[a,b] Q_j[b,c]
//   backward: gPhi_ij = <gA_ij, Q_i Q_j>;  gQ_g = sum_j Phi_gj gA_gj Q_j^T + sum_i Phi_ig Q_i^T gA_ig;
//             galpha: reverse sweep through the Givens chain (a rotation's angle derivative needs the state BEHIND it only:
//             d row_i' = -row_m', d row_m' = row_i'; the state in front of it is R^T times the state behind it).
// One 256-thread workgroup per band; everything (N = G nper <= 32) lives in LDS in float64, so that forward and adjoint carry
// the float32 rounding of their inputs and outputs only.  A left multiplication by a rotation acts on every COLUMN of U on
// its own: thread j < G keeps column j and walks the whole chain without a barrier.  No atomics, fixed summation orders:
// the same inputs give the same bits, and a band's result does not depend on the other bands of the launch.
// The torch build of the same matrices issues dozens of tiny launches per band (ND_Unitary's recursion, einsum, kron).
#include "common.h"

#define CPL_MAXN GFDN_MAX_BLOCK
#define CPL_MAXG GFDN_MAX_GROUPS
#define CPL_MAXP (CPL_MAXG * (CPL_MAXG - 1) / 2)
#define CPL_PI_F 3.14159274101257324f      // float32(pi): what torch.clamp(alpha_f32, -np.pi, np.pi) clamps to

// (cos, sin) of the band's clamped angles -> cs[2 k], cs[2 k + 1]
__device__ __forceinline__ void cpl_angles(const float* __restrict__ alpha, int npairs, double* cs) {
  for (int k = threadIdx.x; k < npairs; k += blockDim.x) {
    const float a = fminf(fmaxf(alpha[k], -CPL_PI_F), CPL_PI_F);
    double s, c;
    sincos((double)a, &s, &c);
    cs[2 * k] = c;
    cs[2 * k + 1] = s;
  }
}

// U (G x G, row-major in LDS) <- Phi; thread j < G owns column j.  Rotation k = (m-1)(m-2)/2 + i, m = 2 .. G, i = 0 .. m-2,
// acts on rows (i, m-1): row_i' = c row_i - s row_m, row_m' = s row_i + c row_m.
__device__ __forceinline__ void cpl_phi_column(const double* cs, int G, int j, double* U) {
  double col[CPL_MAXG];
#pragma unroll
  for (int r = 0; r < CPL_MAXG; ++r) col[r] = (r == j) ? 1.0 : 0.0;
  int k = 0;
  for (int m = 2; m <= G; ++m)
    for (int i = 0; i < m - 1; ++i, ++k) {
      const double c = cs[2 * k], s = cs[2 * k + 1];
      double ri = 0.0, rm = 0.0;
#pragma unroll
      for (int r = 0; r < CPL_MAXG; ++r) {
        ri = (r == i) ? col[r] : ri;
        rm = (r == m - 1) ? col[r] : rm;
      }
      const double ni = c * ri - s * rm, nm = s * ri + c * rm;
#pragma unroll
      for (int r = 0; r < CPL_MAXG; ++r) col[r] = (r == i) ? ni : ((r == m - 1) ? nm : col[r]);
    }
#pragma unroll
  for (int r = 0; r < CPL_MAXG; ++r)
    if (r < G) U[r * G + j] = col[r];
}

__global__ __launch_bounds__(256) void k_coupled_feedback_fwd(const float* __restrict__ Q, const float* __restrict__ alpha,
                                                              int G, int n, float* __restrict__ A,
                                                              float* __restrict__ Phi) {
  __shared__ double sQ[CPL_MAXN * CPL_MAXN];
  __shared__ double sU[CPL_MAXG * CPL_MAXG];
  __shared__ double cs[2 * CPL_MAXP + 2];
  const int band = blockIdx.x, N = G * n, npairs = G * (G - 1) / 2;
  const float* Qb = Q + (size_t)band * G * n * n;
  for (int e = threadIdx.x; e < G * n * n; e += blockDim.x) sQ[e] = (double)Qb[e];
  cpl_angles(alpha + (size_t)band * npairs, npairs, cs);
  __syncthreads();
  if (threadIdx.x < G) cpl_phi_column(cs, G, threadIdx.x, sU);
  __syncthreads();
  for (int e = threadIdx.x; e < G * G; e += blockDim.x) Phi[(size_t)band * G * G + e] = (float)sU[e];
  float* Ab = A + (size_t)band * N * N;
  for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
    const int r = e / N, q = e - r * N;
    const int i = r / n, a = r - i * n, j = q / n, c = q - j * n;
    const double* Qi = sQ + i * n * n + a * n;
    const double* Qj = sQ + j * n * n + c;
    double acc = 0.0;
    for (int b = 0; b < n; ++b) acc += Qi[b] * Qj[b * n];
    // (G = 1: the reference returns block_M unscaled, and Phi = [[1]] here)
    Ab[e] = (float)(G == 1 ? acc : sU[i * G + j] * acc);
  }
}

__global__ __launch_bounds__(256) void k_coupled_feedback_bwd(const float* __restrict__ Q, const float* __restrict__ alpha,
                                                              int G, int n, const float* __restrict__ gA,
                                                              float* __restrict__ gQ, float* __restrict__ galpha) {
  __shared__ double sQ[CPL_MAXN * CPL_MAXN];
  __shared__ double sG[CPL_MAXN * CPL_MAXN];       // gA of the band
  __shared__ double sP[CPL_MAXN * CPL_MAXN];       // block (i,j) = Q_i Q_j
  __shared__ double sU[CPL_MAXG * CPL_MAXG];
  __shared__ double sgU[CPL_MAXG * CPL_MAXG];
  __shared__ double cs[2 * CPL_MAXP + 2];
  __shared__ double part[256];
  __shared__ double gpart[CPL_MAXP * CPL_MAXG + 1];
  const int band = blockIdx.x, N = G * n, npairs = G * (G - 1) / 2;
  const float* Qb = Q + (size_t)band * G * n * n;
  const float* gAb = gA + (size_t)band * N * N;
  for (int e = threadIdx.x; e < G * n * n; e += blockDim.x) sQ[e] = (double)Qb[e];
  for (int e = threadIdx.x; e < N * N; e += blockDim.x) sG[e] = (double)gAb[e];
  cpl_angles(alpha + (size_t)band * npairs, npairs, cs);
  __syncthreads();
  if (threadIdx.x < G) cpl_phi_column(cs, G, threadIdx.x, sU);
  for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
    const int r = e / N, q = e - r * N;
    const int i = r / n, a = r - i * n, j = q / n, c = q - j * n;
    const double* Qi = sQ + i * n * n + a * n;
    const double* Qj = sQ + j * n * n + c;
    double acc = 0.0;
    for (int b = 0; b < n; ++b) acc += Qi[b] * Qj[b * n];
    sP[e] = acc;
  }
  __syncthreads();
  // dL/dQ_g[a,b] = sum_j Phi_gj sum_c gA_gj[a,c] Q_j[b,c]  +  sum_i Phi_ig sum_a' Q_i[a',a] gA_ig[a',b]
  float* gQb = gQ + (size_t)band * G * n * n;
  for (int e = threadIdx.x; e < G * n * n; e += blockDim.x) {
    const int g = e / (n * n), ab = e - g * n * n, a = ab / n, b = ab - a * n;
    double acc = 0.0;
    for (int j = 0; j < G; ++j) {
      const double* gr = sG + (g * n + a) * N + j * n;        // row a of gA_gj
      const double* qr = sQ + j * n * n + b * n;              // row b of Q_j
      double t = 0.0;
      for (int c = 0; c < n; ++c) t += gr[c] * qr[c];
      acc += (G == 1 ? 1.0 : sU[g * G + j]) * t;
    }
    for (int i = 0; i < G; ++i) {
      const double* qc = sQ + i * n * n + a;                  // column a of Q_i
      const double* gc = sG + (i * n) * N + g * n + b;        // column b of gA_ig
      double t = 0.0;
      for (int ap = 0; ap < n; ++ap) t += qc[ap * n] * gc[ap * N];
      acc += (G == 1 ? 1.0 : sU[i * G + g]) * t;
    }
    gQb[e] = (float)acc;
  }
  if (G == 1) return;                                          // (uniform: no angles, nothing behind this point for G = 1)
  // dL/dPhi_ij = <gA_ij, Q_i Q_j>: T threads per pair, partial sums in a fixed order
  const int GG = G * G;
  int T = 256 / GG;
  T = T > 16 ? 16 : T;
  {
    const int p = threadIdx.x / T, l = threadIdx.x - p * T;
    if (p < GG) {
      const int i = p / G, j = p - i * G;
      double acc = 0.0;
      for (int e = l; e < n * n; e += T) {
        const int a = e / n, c = e - a * n;
        const int at = (i * n + a) * N + j * n + c;
        acc += sG[at] * sP[at];
      }
      part[p * T + l] = acc;
    }
  }
  __syncthreads();
  if (threadIdx.x < GG) {
    double acc = 0.0;
    for (int l = 0; l < T; ++l) acc += part[threadIdx.x * T + l];
    sgU[threadIdx.x] = acc;
  }
  __syncthreads();
  // reverse sweep: thread j < G walks column j of (U, gU) back through the chain
  if (threadIdx.x < G) {
    const int j = threadIdx.x;
    double u[CPL_MAXG], gu[CPL_MAXG];
#pragma unroll
    for (int r = 0; r < CPL_MAXG; ++r) {
      u[r] = r < G ? sU[r * G + j] : 0.0;
      gu[r] = r < G ? sgU[r * G + j] : 0.0;
    }
    int k = npairs - 1;
    for (int m = G; m >= 2; --m)
      for (int i = m - 2; i >= 0; --i, --k) {
        const double c = cs[2 * k], s = cs[2 * k + 1];
        double ui = 0.0, um = 0.0, gi = 0.0, gm = 0.0;
#pragma unroll
        for (int r = 0; r < CPL_MAXG; ++r) {
          ui = (r == i) ? u[r] : ui;
          um = (r == m - 1) ? u[r] : um;
          gi = (r == i) ? gu[r] : gi;
          gm = (r == m - 1) ? gu[r] : gm;
        }
        gpart[k * G + j] = gm * ui - gi * um;
        const double pui = c * ui + s * um, pum = c * um - s * ui;       // R^T: the state in front of the rotation
        const double pgi = c * gi + s * gm, pgm = c * gm - s * gi;
#pragma unroll
        for (int r = 0; r < CPL_MAXG; ++r) {
          u[r] = (r == i) ? pui : ((r == m - 1) ? pum : u[r]);
          gu[r] = (r == i) ? pgi : ((r == m - 1) ? pgm : gu[r]);
        }
      }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < npairs; k += blockDim.x) {
    double acc = 0.0;
    for (int j = 0; j < G; ++j) acc += gpart[k * G + j];
    // the clamp's gradient: one on the closed interval, zero outside (torch.clamp)
    const float a = alpha[(size_t)band * npairs + k];
    galpha[(size_t)band * npairs + k] = (a >= -CPL_PI_F && a <= CPL_PI_F) ? (float)acc : 0.0f;
  }
}

static int coupled_args(int nbands, int G, int nper) {
  if (nbands <= 0 || G <= 0 || nper <= 0) return GFDN_E_BADARG;
  if (G > GFDN_MAX_GROUPS || (long long)G * nper > GFDN_MAX_BLOCK) return GFDN_E_UNSUPPORTED;
  return 0;
}

extern "C" int gfdn_coupled_feedback_fwd(const float* Q, const float* alpha, int nbands, int G, int nper, float* A,
                                         float* Phi, void* stream) {
  if (!Q || !A || !Phi || (!alpha && G > 1)) return GFDN_E_BADARG;
  int rc = coupled_args(nbands, G, nper);
  if (rc) return rc;
  hipLaunchKernelGGL(k_coupled_feedback_fwd, dim3(nbands), dim3(256), 0, (hipStream_t)stream, Q, alpha, G, nper, A, Phi);
  GFDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gfdn_coupled_feedback_bwd(const float* Q, const float* alpha, int nbands, int G, int nper, const float* gA,
                                         float* gQ, float* galpha, void* stream) {
  if (!Q || !gA || !gQ || ((!alpha || !galpha) && G > 1)) return GFDN_E_BADARG;
  int rc = coupled_args(nbands, G, nper);
  if (rc) return rc;
  hipLaunchKernelGGL(k_coupled_feedback_bwd, dim3(nbands), dim3(256), 0, (hipStream_t)stream, Q, alpha, G, nper, gA, gQ,
                     galpha);
  GFDN_LAUNCH_CHECK();
  return 0;
}
