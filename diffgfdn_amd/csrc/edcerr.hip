// EDC matching error of a band bank's render for gfx950: every (receiver, analysis band) in one pass.
//
// reference: plot.py:606-757 ``plot_edc_error_in_space`` -> ``get_edc_error`` (:632-661): octave-filter the measured and the
// estimated RIRs, Schroeder backward integral of each band (normalize = False), dB (utils.py:16-40: 10 log10(|v| + eps_f32),
// floor -200), mean over time of the absolute difference per receiver and band.  The analysis filter is linear, so for a bank
//     a_k * y[r] = a_k * D[r] + sum_s W[r][s] (a_k * C_s)
// (DESIGN 5.1.3): Dk (R_store, A, ld) is a constant of the dataset and the taps, Ck (A, S, ld_c) are S signals per analysis
// band whatever R is, and the estimate's band signals exist only in registers here:
//     x[t] = Dk[row][k][t] + sum_{s < S} W[r][s] Ck[k][s][t],   E[t] = sum_{u >= t} x[u]^2,   dB(E[t]),   t < L
//     mode 0 (error):  err[r][k] = (1 / L) sum_t |dB(E[t]) - Tdb[row][k][t]|
//     mode 1 (curve):  out[r][k][t] = dB(E[t])                  (how Tdb is built, S = 0: both sides take the same arithmetic)
//
// Tiling.  A 256-thread workgroup owns one analysis band k and a group of RG <= 16 receivers and walks the tiles of
// EE_TILE = 1024 samples BACKWARDS from the row's end; thread l holds samples 4 l .. 4 l + 3 of the tile.  Per tile it loads
// the tile of the band's S signals into registers once (ST x 4 VGPRs, ST = S rounded up to 8 / 16 / 24 / 32 as in
// render.hip; ST = 0: Dk already is the band signal) for the whole group: the L2 -> CU stream of the group signals, which
// binds the one-receiver-per-workgroup form (csrc/edcone.hip), is paid once per RG receivers.  The receivers go
// in batches of EE_RB = 4 with ONE barrier per batch: compose (acc = d, then fma(w_s, c_s, acc), s = 0 .. S-1), square,
// suffix sums of the thread's four samples, suffix scan over the wave on the VALU (DPP: wave_scan_incl_rev), the four wave
// totals of every receiver of the batch to LDS, barrier, then every thread adds the totals of the waves behind its own and
// the receiver's carry and takes the dB stage.
//
// Summation order and precision.  Inside a tile the sums are float32 in the fixed order above; the carry over the tiles
// behind is a float64 per receiver in LDS (two copies, alternating per tile; thread 0 writes the next tile's while the
// others read this tile's), added to the tile's float32 suffix in float64 and rounded once.  The per-thread |difference|
// sums go to float64 accumulators in LDS (one per receiver and thread) and are added up over the threads in index order
// by one thread per receiver.  No atomics: a receiver's result does not depend on which group or launch it is in, so a
// call repeats bit for bit and a ``rows`` subset gives the bits of the same rows of the full call.
//
// Alignment.  16-byte accesses when Dk, Ck, Tdb / out are 16-byte aligned and their pitches multiples of four floats;
// otherwise the same kernel with 4-byte accesses of the same samples (the same bits).  The partial last tile (the first
// one walked) always takes 4-byte accesses with its load addresses clamped to the row and its stores guarded: nothing is
// read or written behind sample L - 1 of a row.  Plain vector stores only.
#include "common.h"

#define EE_THREADS 256
#define EE_TILE (4 * EE_THREADS)
#define EE_MAX_S 32
#define EE_RB 4
#define EE_MAX_RG 16
#define EE_MIN_WGS 512
#define EE_ACC_PITCH (EE_THREADS + 1)
#define TEN_LOG10_2 3.0102999566398120f

typedef float ee_f2 __attribute__((ext_vector_type(2)));
typedef float ee_f4 __attribute__((ext_vector_type(4)));

// the thread's four consecutive samples t0 .. t0 + 3 of row ``p``.  ``vec``: one 16-byte access (full tile, aligned rows);
// else four 4-byte loads with t clamped to the row's last sample (the caller zeroes what lies behind it)
template <int VEC>
__device__ __forceinline__ ee_f4 ee_load(const float* __restrict__ p, long long t0, int L, bool full) {
  if (VEC == 4 && full) return *reinterpret_cast<const ee_f4*>(p + t0);
  ee_f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    long long t = t0 + e;
    if (t > L - 1) t = L - 1;
    v[e] = p[t];
  }
  return v;
}
template <int VEC>
__device__ __forceinline__ void ee_store(float* __restrict__ p, long long t0, int L, bool full, ee_f4 v) {
  if (VEC == 4 && full) {
    *reinterpret_cast<ee_f4*>(p + t0) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (t0 + e < L) p[t0 + e] = v[e];
}

// d + sum_s wi[s] c_s in the order s = 0 .. S-1 (render.hip's rm_mix: rows s >= S of the tile are zero and meet the last
// weight again)
template <int ST>
__device__ __forceinline__ ee_f4 ee_mix(ee_f4 dv, const ee_f4* cr, const float* __restrict__ wi, int S) {
  if (ST == 0) return dv;
  float ws[ST ? ST : 1];
#pragma unroll
  for (int s = 0; s < ST; ++s) ws[s] = wi[s < ST - 8 ? s : (s < S ? s : S - 1)];
  ee_f2 lo = {dv[0], dv[1]}, hi = {dv[2], dv[3]};
#pragma unroll
  for (int s = 0; s < ST; ++s) {
    const ee_f2 w2 = {ws[s], ws[s]};
    lo = __builtin_elementwise_fma(w2, (ee_f2){cr[s][0], cr[s][1]}, lo);
    hi = __builtin_elementwise_fma(w2, (ee_f2){cr[s][2], cr[s][3]}, hi);
  }
  return (ee_f4){lo[0], lo[1], hi[0], hi[1]};
}

// 10 log10(|v| + eps_f32), floor -200 (utils.py:16-40) on the hardware's base-2 logarithm (v_log_f32, one ulp; its
// argument is at least eps_f32: never a denormal)
__device__ __forceinline__ float ee_db(float v) {
  return fmaxf(TEN_LOG10_2 * __builtin_amdgcn_logf(fabsf(v) + F32_EPS), -200.0f);
}

// grid: A x groups workgroups, the group fastest.  MODE 0: error against tdb -> out (R, ld_o >= A); MODE 1: curve -> out
// (R, A, ld_o >= L)
template <int ST, int VEC, int MODE>
__global__ __launch_bounds__(EE_THREADS) void k_edc_err(const float* __restrict__ dk, size_t ld_d,
                                                        const long long* __restrict__ rows, const float* __restrict__ w,
                                                        const float* __restrict__ ck, size_t ld_c,
                                                        const float* __restrict__ tdb, size_t ld_t, int R, int A, int S,
                                                        int L, int RG, int groups, float* __restrict__ out, size_t ld_o) {
  __shared__ double s_carry[2][EE_MAX_RG];
  __shared__ float s_tot[2][EE_RB][4];
  __shared__ double s_acc[MODE == 0 ? EE_MAX_RG * EE_ACC_PITCH : 1];
  const int tid = threadIdx.x, wv = tid >> 6;
  const int k = blockIdx.x / groups;
  const int g0 = (blockIdx.x % groups) * RG;
  const int g1 = g0 + RG < R ? g0 + RG : R;               // receivers g0 .. g1 - 1
  if (tid < EE_MAX_RG) s_carry[0][tid] = s_carry[1][tid] = 0.0;
  if (MODE == 0)
    for (int j = 0; j < EE_MAX_RG; ++j) s_acc[j * EE_ACC_PITCH + tid] = 0.0;
  __syncthreads();

  const int tiles = (L + EE_TILE - 1) / EE_TILE;
  const float* ckk = ST ? ck + (size_t)k * S * ld_c : nullptr;
  int buf = 0, par = 0;
  for (int it = tiles - 1; it >= 0; --it, par ^= 1) {
    const long long t0 = (long long)it * EE_TILE + 4 * tid;
    const bool full = (long long)(it + 1) * EE_TILE <= L;
    ee_f4 cr[ST ? ST : 1];
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      // (rows s >= S: a valid row is loaded and dropped, as in render.hip)
      const ee_f4 v = ee_load<VEC>(ckk + (size_t)(s < ST - 8 || s < S ? s : S - 1) * ld_c, t0, L, full);
      cr[s] = (s < ST - 8 || s < S) ? v : (ee_f4){0.f, 0.f, 0.f, 0.f};
    }
    for (int b0 = g0; b0 < g1; b0 += EE_RB, buf ^= 1) {
      ee_f4 v[EE_RB], tq[EE_RB];
      // ---- compose, square, scan inside the wave; the wave totals of the batch to LDS
#pragma unroll
      for (int j = 0; j < EE_RB; ++j) {
        const int ic = b0 + j < g1 ? b0 + j : g1 - 1;      // (behind the group: the last receiver again, dropped below)
        const size_t row = rows ? (size_t)rows[ic] : (size_t)ic;
        const ee_f4 dv = ee_load<VEC>(dk + (row * A + k) * ld_d, t0, L, full);
        if (MODE == 0) tq[j] = ee_load<VEC>(tdb + (row * A + k) * ld_t, t0, L, full);
        ee_f4 x = ee_mix<ST>(dv, cr, ST ? w + (size_t)ic * S : nullptr, S);
        ee_f4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = t0 + e < L ? x[e] * x[e] : 0.f;
        q[2] += q[3];
        q[1] += q[2];
        q[0] += q[1];                                       // q[e] = sum of the thread's samples e .. 3
        float total;
        const float behind = wave_scan_incl_rev(q[0], total) - q[0];     // the lanes behind this one
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] = q[e] + behind;
        if ((tid & 63) == 0) s_tot[buf][j][wv] = total;
      }
      __syncthreads();
      // ---- the waves behind, the carry of the tiles behind, dB, |difference| or store
#pragma unroll
      for (int j = 0; j < EE_RB; ++j) {
        const int i = b0 + j;
        if (i >= g1) break;
        const float w0 = s_tot[buf][j][0], w1 = s_tot[buf][j][1], w2 = s_tot[buf][j][2], w3 = s_tot[buf][j][3];
        const float later = wv == 3 ? 0.f : (wv == 2 ? w3 : (wv == 1 ? w3 + w2 : (w3 + w2) + w1));
        const double carry = s_carry[par][i - g0];
        if (tid == 0) s_carry[par ^ 1][i - g0] = carry + (double)(((w3 + w2) + w1) + w0);
        ee_f4 db;
#pragma unroll
        for (int e = 0; e < 4; ++e) db[e] = ee_db((float)(carry + (double)(v[j][e] + later)));
        if (MODE == 0) {
          float a = 0.f;
#pragma unroll
          for (int e = 3; e >= 0; --e) a += t0 + e < L ? fabsf(db[e] - tq[j][e]) : 0.f;
          s_acc[(i - g0) * EE_ACC_PITCH + tid] += (double)a;
        } else {
          ee_store<VEC>(out + ((size_t)i * A + k) * ld_o, t0, L, full, db);
        }
      }
    }
  }
  if (MODE == 0) {
    __syncthreads();
    if (tid < g1 - g0) {                                    // one thread per receiver: the threads' sums in index order
      double sum = 0.0;
      for (int l = 0; l < EE_THREADS; ++l) sum += s_acc[tid * EE_ACC_PITCH + l];
      out[(size_t)(g0 + tid) * ld_o + k] = (float)(sum / (double)L);
    }
  }
}

template <int ST, int VEC>
static void ee_launch2(int mode, unsigned grid, hipStream_t st, const float* dk, size_t ld_d, const long long* rows,
                       const float* w, const float* ck, size_t ld_c, const float* tdb, size_t ld_t, int R, int A, int S,
                       int L, int RG, int groups, float* out, size_t ld_o) {
  if (mode == 0)
    hipLaunchKernelGGL((k_edc_err<ST, VEC, 0>), dim3(grid), dim3(EE_THREADS), 0, st, dk, ld_d, rows, w, ck, ld_c, tdb, ld_t,
                       R, A, S, L, RG, groups, out, ld_o);
  else
    hipLaunchKernelGGL((k_edc_err<ST, VEC, 1>), dim3(grid), dim3(EE_THREADS), 0, st, dk, ld_d, rows, w, ck, ld_c, tdb, ld_t,
                       R, A, S, L, RG, groups, out, ld_o);
}
template <int ST>
static void ee_launch(bool vec, int mode, unsigned grid, hipStream_t st, const float* dk, size_t ld_d, const long long* rows,
                      const float* w, const float* ck, size_t ld_c, const float* tdb, size_t ld_t, int R, int A, int S, int L,
                      int RG, int groups, float* out, size_t ld_o) {
  if (vec)
    ee_launch2<ST, 4>(mode, grid, st, dk, ld_d, rows, w, ck, ld_c, tdb, ld_t, R, A, S, L, RG, groups, out, ld_o);
  else
    ee_launch2<ST, 1>(mode, grid, st, dk, ld_d, rows, w, ck, ld_c, tdb, ld_t, R, A, S, L, RG, groups, out, ld_o);
}

extern "C" int gfdn_edc_err(const float* dk, int ld_d, const long long* rows, const float* w, const float* ck, int ld_c,
                            const float* tdb, int ld_t, int R, int A, int S, int L, int mode, float* out, int ld_o,
                            void* stream) {
  if (!dk || !out || R <= 0 || A <= 0 || S < 0 || L <= 0 || ld_d < L) return GFDN_E_BADARG;
  if ((w == nullptr) != (ck == nullptr) || (S > 0) != (ck != nullptr)) return GFDN_E_BADARG;
  if (S > 0 && ld_c < L) return GFDN_E_BADARG;
  if (mode == 0) {
    if (!tdb || ld_t < L || ld_o < A) return GFDN_E_BADARG;
  } else if (mode == 1) {
    if (ld_o < L) return GFDN_E_BADARG;
  } else {
    return GFDN_E_BADARG;
  }
  if (S > EE_MAX_S) return GFDN_E_UNSUPPORTED;
  // receivers per workgroup: 16, halved down to one batch while the launch has fewer than EE_MIN_WGS workgroups
  int RG = EE_MAX_RG;
  while (RG > EE_RB && (long long)A * ((R + RG - 1) / RG) < EE_MIN_WGS) RG >>= 1;
  const int groups = (R + RG - 1) / RG;
  if ((long long)A * groups > 0x7fffffffLL) return GFDN_E_UNSUPPORTED;
  bool vec = (((uintptr_t)dk | (uintptr_t)ck) & 15) == 0 && ((ld_d | (S ? ld_c : 0)) & 3) == 0;
  if (mode == 0)
    vec = vec && ((uintptr_t)tdb & 15) == 0 && (ld_t & 3) == 0;
  else
    vec = vec && ((uintptr_t)out & 15) == 0 && (ld_o & 3) == 0;
  const unsigned grid = (unsigned)((long long)A * groups);
  hipStream_t st = (hipStream_t)stream;
#define EE_GO(ST)                                                                                                     \
  ee_launch<ST>(vec, mode, grid, st, dk, (size_t)ld_d, rows, w, ck, (size_t)ld_c, tdb, (size_t)ld_t, R, A, S, L, RG, \
                groups, out, (size_t)ld_o)
  if (S == 0)
    EE_GO(0);
  else if (S <= 8)
    EE_GO(8);
  else if (S <= 16)
    EE_GO(16);
  else if (S <= 24)
    EE_GO(24);
  else
    EE_GO(32);
#undef EE_GO
  GFDN_LAUNCH_CHECK();
  return 0;
}
