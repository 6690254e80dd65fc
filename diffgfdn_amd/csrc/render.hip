// Full-band render mix of a band bank for gfx950: every receiver's room impulse response as ONE skinny product.
//
// reference: run_subband_training_treble.py:207-375 (``inferencing``): per band and receiver get_response (utils.py:149-179:
// h = irfft(H)), fftconvolve(h, taps, 'full') (:321-324), sum over the bands per receiver (:358).  Neither transform depends
// on the receiver, which enters only through its G gains per band (model.py:583-619):
//     y[r] = D[r] + sum_s W[r][s] C[s],    s = band G + g,  C[s] = irfft(T_s) (*) taps_band,  D[r] = sum_bands irfft(d) (*) taps
// D is a constant of the dataset, C are the bank's S = bands x G filtered group signals: this file is the product
//     out[i][t] = d[rows ? rows[i] : i][t] + sum_{s < S} w[i S + s] c[s][t]        (float32, i < R, t < n).
//
// Tiling.  A 256-thread workgroup owns a tile of RM_TILE = 1024 samples -- 16 bytes per lane, so that d and out move as
// dwordx4 -- and a run of receivers.  It loads the tile of all S signals into registers ONCE (ST x 4 VGPRs, ST = S rounded up
// to 8 / 16 / 24 / 32: the array is indexed by unrolled loops only, rows s >= S hold zeros and meet zero weights) and walks
// its receivers: per receiver one 16-byte load, ST x 2 packed FMAs (v_pk_fma_f32) and one 16-byte store per lane.  The
// receiver index is the same for the whole workgroup, so its S weights (and rows[i]) are scalar loads into SGPRs.  A queue
// of RM_PF = 3 rows of d stays in flight ahead of the receiver being mixed; at ST = 32 the tile (128 VGPRs), the queue and
// the accumulators fit the 168 VGPRs of three waves per SIMD.  acc = d, then acc = fma(w_s, c_s, acc) for s = 0 .. S-1 in
// that order: S roundings per sample, the same bits whatever the split (the rows / chunk arguments of the callers rely
// on it).
//
// Receiver split.  The receivers are cut into runs so that the launch has about RM_GRID_WGS = 2048 workgroups: eight per
// CU of the 256, i.e. between two and three rounds of the 768 that fit at once (three workgroups per CU at the ST = 32
// register count).  At the headline shape (R = 838, n = 131 200: 129 tiles) that is 16 runs of 53 receivers.  More runs
// would fill the tail of the launch better but every run re-reads its tile of C: S x 16 bytes per lane against the 32
// bytes per lane and receiver that d and out move, i.e. S / (2 run) of the compulsory traffic -- 26 % at 53 receivers and
// S = 28, twice that at half the run; never fewer than RM_MIN_RUN = 8 receivers per run.  Those re-reads are meant to hit
// L2 / Infinity Cache, not HBM (C is S n floats, 14.7 MB at the headline shape): the run is the FASTEST-varying part of
// the workgroup index, so the workgroups that share a tile are dispatched back to back.
//
// Alignment.  The 16-byte path needs d, c, out 16-byte aligned with pitches that are multiples of four floats; everything
// else takes the same kernel with 4-byte accesses (lane l: samples l, l + 256, l + 512, l + 768 of the tile: still
// coalesced).  A partial last tile always runs that form with its addresses clamped to the row (loads) and its stores
// guarded: no access past sample n - 1 of any row.  Plain vector stores only; a thread writes exactly the elements it read
// from d, so out may be d itself (rows = NULL), which is how the callers chain launches for S > 32.
#include "common.h"

#define RM_THREADS 256
#define RM_TILE (4 * RM_THREADS)
#define RM_MAX_S 32
#define RM_GRID_WGS 2048
#define RM_PF 3
#define RM_MIN_RUN 8

typedef float rm_f2 __attribute__((ext_vector_type(2)));
typedef float rm_f4 __attribute__((ext_vector_type(4)));

// the thread's four samples of row ``p`` (VEC = 4: consecutive, one 16-byte access; VEC = 1: strided by the workgroup).
// FULL = false: t0 + the offset is clamped to the row's last sample (the value is never stored)
template <int VEC, bool FULL>
__device__ __forceinline__ rm_f4 rm_load(const float* p, long long t0, int n) {
  if (VEC == 4) return *reinterpret_cast<const rm_f4*>(p + t0);
  rm_f4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    long long t = t0 + (long long)j * RM_THREADS;
    if (!FULL && t > n - 1) t = n - 1;
    v[j] = p[t];
  }
  return v;
}
template <int VEC, bool FULL>
__device__ __forceinline__ void rm_store(float* p, long long t0, int n, rm_f4 v) {
  if (VEC == 4) {
    *reinterpret_cast<rm_f4*>(p + t0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long t = t0 + (long long)j * RM_THREADS;
    if (FULL || t < n) p[t] = v[j];
  }
}

// d + sum_s wi[s] c_s in the order s = 0 .. S-1.  ST - 8 < S <= ST: only the last eight can lie behind S; those read the last
// weight again, against a zero row of the tile (no select, and no branch around the scalar loads)
template <int ST>
__device__ __forceinline__ rm_f4 rm_mix(rm_f4 dv, const rm_f4 (&cr)[ST], const float* __restrict__ wi, int S) {
  float ws[ST];
#pragma unroll
  for (int s = 0; s < ST; ++s) ws[s] = wi[s < ST - 8 ? s : (s < S ? s : S - 1)];
  rm_f2 lo = {dv[0], dv[1]}, hi = {dv[2], dv[3]};
#pragma unroll
  for (int s = 0; s < ST; ++s) {
    const rm_f2 w2 = {ws[s], ws[s]};
    lo = __builtin_elementwise_fma(w2, (rm_f2){cr[s][0], cr[s][1]}, lo);
    hi = __builtin_elementwise_fma(w2, (rm_f2){cr[s][2], cr[s][3]}, hi);
  }
  return (rm_f4){lo[0], lo[1], hi[0], hi[1]};
}

template <int ST, int VEC, bool FULL, bool ROWS>
__device__ __forceinline__ void rm_body(const float* d, size_t ld_d, const long long* __restrict__ rows,
                                        const float* __restrict__ w, const float* __restrict__ c, size_t ld_c, int S, int n,
                                        int r0, int r1, float* out, size_t ld_out, long long t0) {
  rm_f4 cr[ST];
#pragma unroll
  for (int s = 0; s < ST; ++s) {
    // (rows s >= S: a valid row is loaded and dropped -- a branch around the load would serialise the ST loads)
    const rm_f4 v = rm_load<VEC, FULL>(c + (size_t)(s < ST - 8 || s < S ? s : S - 1) * ld_c, t0, n);
    cr[s] = (s < ST - 8 || s < S) ? v : (rm_f4){0.f, 0.f, 0.f, 0.f};
  }
  // a queue of RM_PF rows of d in flight ahead of the receiver being mixed (unrolled: static register indices); the loads
  // behind the run's last receiver are clamped to it and dropped.  In place (out = d) a row is loaded before the pass that
  // stores it, by the thread that stores it.
  rm_f4 q[RM_PF];
#pragma unroll
  for (int j = 0; j < RM_PF; ++j) {
    const int ip = r0 + j < r1 ? r0 + j : r1 - 1;
    q[j] = rm_load<VEC, FULL>(d + (ROWS ? (size_t)rows[ip] : (size_t)ip) * ld_d, t0, n);
  }
  int i = r0;
  for (; i + RM_PF <= r1; i += RM_PF) {
#pragma unroll
    for (int j = 0; j < RM_PF; ++j) {
      const int ic = i + j;
      const rm_f4 dv = q[j];
      const int ip = ic + RM_PF < r1 ? ic + RM_PF : r1 - 1;
      q[j] = rm_load<VEC, FULL>(d + (ROWS ? (size_t)rows[ip] : (size_t)ip) * ld_d, t0, n);
      rm_store<VEC, FULL>(out + (size_t)ic * ld_out, t0, n, rm_mix<ST>(dv, cr, w + (size_t)ic * S, S));
    }
  }
#pragma unroll
  for (int j = 0; j < RM_PF - 1; ++j)          // the last r1 - i < RM_PF receivers: their rows are in the queue
    if (i + j < r1) rm_store<VEC, FULL>(out + (size_t)(i + j) * ld_out, t0, n, rm_mix<ST>(q[j], cr, w + (size_t)(i + j) * S, S));
}

// grid: tiles x runs workgroups, the run fastest.  d and out may be the same buffer: not __restrict__
// (three waves per SIMD: 168 VGPRs, which the ST = 32 form fits with its queue)
template <int ST, int VEC, bool ROWS>
__global__ __launch_bounds__(RM_THREADS, 3) void k_render_mix(const float* d, size_t ld_d, const long long* __restrict__ rows,
                                                           const float* __restrict__ w, const float* __restrict__ c,
                                                           size_t ld_c, int R, int S, int n, int runs, int run_len,
                                                           float* out, size_t ld_out) {
  const int run = blockIdx.x % runs;
  const long long tile0 = (long long)(blockIdx.x / runs) * RM_TILE;
  const int r0 = run * run_len;
  const int r1 = r0 + run_len < R ? r0 + run_len : R;
  if (tile0 + RM_TILE <= n)
    rm_body<ST, VEC, true, ROWS>(d, ld_d, rows, w, c, ld_c, S, n, r0, r1, out, ld_out,
                           tile0 + (VEC == 4 ? 4 * (int)threadIdx.x : (int)threadIdx.x));
  else
    rm_body<ST, 1, false, ROWS>(d, ld_d, rows, w, c, ld_c, S, n, r0, r1, out, ld_out, tile0 + (int)threadIdx.x);
}

template <int ST, int VEC>
static void rm_launch2(unsigned grid, hipStream_t st, const float* d, size_t ld_d, const long long* rows, const float* w,
                       const float* c, size_t ld_c, int R, int S, int n, int runs, int run_len, float* out, size_t ld_out) {
  if (rows)
    hipLaunchKernelGGL((k_render_mix<ST, VEC, true>), dim3(grid), dim3(RM_THREADS), 0, st, d, ld_d, rows, w, c, ld_c, R, S, n,
                       runs, run_len, out, ld_out);
  else
    hipLaunchKernelGGL((k_render_mix<ST, VEC, false>), dim3(grid), dim3(RM_THREADS), 0, st, d, ld_d, rows, w, c, ld_c, R, S, n,
                       runs, run_len, out, ld_out);
}
template <int ST>
static void rm_launch(bool vec, unsigned grid, hipStream_t st, const float* d, size_t ld_d, const long long* rows,
                      const float* w, const float* c, size_t ld_c, int R, int S, int n, int runs, int run_len, float* out,
                      size_t ld_out) {
  if (vec)
    rm_launch2<ST, 4>(grid, st, d, ld_d, rows, w, c, ld_c, R, S, n, runs, run_len, out, ld_out);
  else
    rm_launch2<ST, 1>(grid, st, d, ld_d, rows, w, c, ld_c, R, S, n, runs, run_len, out, ld_out);
}

extern "C" int gfdn_render_mix(const float* d, int ld_d, const long long* rows, const float* w, const float* c,
                               int ld_c, int R, int S, int n, float* out, int ld_out, void* stream) {
  if (!d || !w || !c || !out || R <= 0 || S <= 0 || n <= 0 || ld_d < n || ld_c < n || ld_out < n) return GFDN_E_BADARG;
  if (rows && d == out) return GFDN_E_BADARG;            // (in place: every thread must read the row it writes)
  if (S > RM_MAX_S) return GFDN_E_UNSUPPORTED;
  const long long tiles = ((long long)n + RM_TILE - 1) / RM_TILE;
  // about RM_GRID_WGS workgroups in all, RM_MIN_RUN receivers per run at the least
  long long want = (RM_GRID_WGS + tiles - 1) / tiles;
  if (want > R) want = R;
  int run_len = (int)((R + want - 1) / want);
  if (run_len < RM_MIN_RUN) run_len = R < RM_MIN_RUN ? R : RM_MIN_RUN;
  const int runs = (R + run_len - 1) / run_len;
  if (tiles * runs > 0x7fffffffLL) return GFDN_E_UNSUPPORTED;
  const bool vec = (((uintptr_t)d | (uintptr_t)c | (uintptr_t)out) & 15) == 0 && ((ld_d | ld_c | ld_out) & 3) == 0;
  const unsigned grid = (unsigned)(tiles * runs);
  hipStream_t st = (hipStream_t)stream;
  if (S <= 8)
    rm_launch<8>(vec, grid, st, d, (size_t)ld_d, rows, w, c, (size_t)ld_c, R, S, n, runs, run_len, out, (size_t)ld_out);
  else if (S <= 16)
    rm_launch<16>(vec, grid, st, d, (size_t)ld_d, rows, w, c, (size_t)ld_c, R, S, n, runs, run_len, out, (size_t)ld_out);
  else if (S <= 24)
    rm_launch<24>(vec, grid, st, d, (size_t)ld_d, rows, w, c, (size_t)ld_c, R, S, n, runs, run_len, out, (size_t)ld_out);
  else
    rm_launch<32>(vec, grid, st, d, (size_t)ld_d, rows, w, c, (size_t)ld_c, R, S, n, runs, run_len, out, (size_t)ld_out);
  GFDN_LAUNCH_CHECK();
  return 0;
}
