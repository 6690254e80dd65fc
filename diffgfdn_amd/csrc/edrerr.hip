// EDR matching error of a band bank's render for gfx950: every receiver in one pass.
//
// reference: plot.py:760-874 ``plot_edr_error_in_space`` -> ``get_edr_error`` (:782-822): STFT of the measured and the
// estimated RIRs (losses.py:501-553 ``get_stft_torch``), energy decay relief EDR[f][m] = dB(sum_{tau >= m} |S[f][tau]|^2)
// (losses.py:556-575, dB of utils.py:16-40: 10 log10(|v| + eps_f32), floor -200), mean over frequency and time of the
// absolute difference per receiver.  The STFT is linear, so for a bank
//     STFT(y[r]) = STFT(D[r]) + sum_s W[r][s] STFT(C_s):
// sd (R_store, T, ld_d) complex64 is a constant of the dataset and the taps, sc (S, T, ld_c) are S short-time spectra
// whatever R is, frames-major with the bin fastest, and the estimate's spectrum exists only in registers here:
//     s[m][f] = sd[row][m][f] + sum_{s < S} w[i][s] sc[s][m][f],   E[m][f] = sum_{tau >= m} |s[tau][f]|^2,   dB(E[m][f])
//     mode 0 (error):  out[i] = (1 / (T F)) sum_{m, f} |dB(E[m][f]) - tdb[row][m][f]|
//     mode 1 (curve):  out[i][m][f] = dB(E[m][f])              (how tdb is built, S = 0: both sides take the same arithmetic)
//
// Tiling.  A workgroup is ONE wave: it owns a tile of ER_TILE = 64 bins, one bin per lane, and a run of up to ER_RUN = 16
// receivers, and walks the frames BACKWARDS from the last.  Per frame it loads the tile of the S signals into registers
// once for the whole run (ST x 2 VGPRs, ST = S rounded up to 8 / 16 / 24 / 32 as in render.hip: static indices, rows s >= S
// are zero and meet the last weight again; ST = 0: sd already is the spectrum); the receiver's weights and rows[i] are
// scalar loads.  Per receiver: acc = sd, then one fma per signal on the real and the imaginary part, s ascending;
// p = fma(im, im, re re); E += p -- the tail sum from the last frame towards the first, at most a few dozen float32 terms,
// smallest first; the dB stage; |difference| into the lane's float64 accumulator of that receiver.  The bins are
// independent: no cross-lane scan, no LDS, no barrier.  The run's E and accumulators are registers (the receiver loop is
// unrolled; slots behind the run's end compute the run's last receiver again and are dropped).
//
// Summation order.  A lane's |differences| are added over the frames in float64; the 64 lanes by a butterfly in float64
// (lanes behind bin F - 1 hold zero); the tile's sum of receiver i goes to work[i tiles + tile], and a second small launch
// adds the tiles of a receiver in index order, scales by 1 / (T F) and rounds once.  No atomics: a receiver's bits depend
// neither on the other receivers of the launch, nor on the run split, nor on ``rows``.
//
// Runs.  The run length is chosen for about ER_GRID_WGS = 2048 waves in the launch, between ER_MIN_RUN and ER_RUN
// receivers: 33 tiles x 60 runs of 14 at the headline shape (838 receivers, 2049 bins).  The run index is the FASTEST part of
// the workgroup index, so the runs of one tile are dispatched back to back and re-read sc from L2.
//
// Alignment.  One complex bin per lane is an 8-byte access (a wave moves 512 contiguous bytes) when sd and sc are 8-byte
// aligned; otherwise the same kernel with two 4-byte accesses per bin (the same bits).  tdb and out move 4 bytes per lane.
// Lanes behind bin F - 1 load bin F - 1 again and store nothing: nothing is read or written behind bin F - 1 of a row.
// Plain vector stores only.
#include "common.h"

#define ER_TILE 64
#define ER_RUN 16
#define ER_MIN_RUN 4
#define ER_MAX_S 32
#define ER_GRID_WGS 2048
#define TEN_LOG10_2 3.0102999566398120f

// bin f of a frame row ``p`` (complex64 as float pairs).  VEC = 2: one 8-byte access; VEC = 1: two 4-byte accesses
template <int VEC>
__device__ __forceinline__ float2 er_load(const float* __restrict__ p, int f) {
  if (VEC == 2) return *reinterpret_cast<const float2*>(p + 2 * (size_t)f);
  return make_float2(p[2 * (size_t)f], p[2 * (size_t)f + 1]);
}

// 10 log10(|v| + eps_f32), floor -200 (utils.py:16-40) on the hardware's base-2 logarithm (v_log_f32, one ulp; its
// argument is at least eps_f32: never a denormal) -- csrc/edcerr.hip's dB stage
__device__ __forceinline__ float er_db(float v) {
  return fmaxf(TEN_LOG10_2 * __builtin_amdgcn_logf(fabsf(v) + F32_EPS), -200.0f);
}

// the sum over the wave's 64 lanes in a fixed order, the same bits in every lane
__device__ __forceinline__ double er_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid: tiles x runs waves, the run fastest.  MODE 0: the tiles' partial sums -> work (R, tiles) float64; MODE 1: curve ->
// out (R, T, ld_o)
template <int ST, int VEC, int MODE>
__global__ __launch_bounds__(ER_TILE) void k_edr_err(const float* __restrict__ sd, size_t ld_d,
                                                    const long long* __restrict__ rows, const float* __restrict__ w,
                                                    const float* __restrict__ sc, size_t ld_c,
                                                    const float* __restrict__ tdb, size_t ld_t, int R, int T, int F, int S,
                                                    int runs, int run_len, int tiles, float* __restrict__ out, size_t ld_o,
                                                    double* __restrict__ work) {
  const int run = blockIdx.x % runs, tile = blockIdx.x / runs;
  const int r0 = run * run_len;
  const int r1 = r0 + run_len < R ? r0 + run_len : R;       // receivers r0 .. r1 - 1, at most ER_RUN of them
  const int f = tile * ER_TILE + (int)threadIdx.x;
  const bool live = f < F;
  const int fc = live ? f : F - 1;                          // (behind the row: its last bin again, dropped below)

  float E[ER_RUN];
  double acc[ER_RUN];
#pragma unroll
  for (int j = 0; j < ER_RUN; ++j) {
    E[j] = 0.f;
    acc[j] = 0.0;
  }
  for (int m = T - 1; m >= 0; --m) {
    float2 cr[ST ? ST : 1];
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      // (rows s >= S: a valid row is loaded and dropped, as in render.hip)
      const int sr = (s < ST - 8 || s < S) ? s : S - 1;
      const float2 v = er_load<VEC>(sc + 2 * ((size_t)sr * T + m) * ld_c, fc);
      cr[s] = (s < ST - 8 || s < S) ? v : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < ER_RUN; ++j) {
      const int ic = r0 + j < r1 ? r0 + j : r1 - 1;
      const size_t row = rows ? (size_t)rows[ic] : (size_t)ic;
      const float2 d = er_load<VEC>(sd + 2 * (row * T + m) * ld_d, fc);
      float t = 0.f;
      if (MODE == 0) t = tdb[(row * T + m) * ld_t + fc];
      float re = d.x, im = d.y;
      if (ST) {
        const float* __restrict__ wi = w + (size_t)ic * S;
#pragma unroll
        for (int s = 0; s < ST; ++s) {
          const float ws = wi[s < ST - 8 ? s : (s < S ? s : S - 1)];
          re = __fmaf_rn(ws, cr[s].x, re);
          im = __fmaf_rn(ws, cr[s].y, im);
        }
      }
      E[j] = __fadd_rn(E[j], __fmaf_rn(im, im, __fmul_rn(re, re)));
      const float db = er_db(E[j]);
      if (MODE == 0) {
        acc[j] += live ? (double)fabsf(db - t) : 0.0;
      } else {
        if (live && r0 + j < r1) out[((size_t)(r0 + j) * T + m) * ld_o + f] = db;
      }
    }
  }
  if (MODE == 0) {
#pragma unroll
    for (int j = 0; j < ER_RUN; ++j) {
      const double sum = er_wave_sum(acc[j]);
      if (threadIdx.x == 0 && r0 + j < r1) work[(size_t)(r0 + j) * tiles + tile] = sum;
    }
  }
}

// out[i] = (sum of receiver i's tiles in index order) / (T F), rounded once
__global__ __launch_bounds__(256) void k_edr_err_sum(const double* __restrict__ work, int R, int tiles, double cells,
                                                     float* __restrict__ out) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= R) return;
  double sum = 0.0;
  for (int t = 0; t < tiles; ++t) sum += work[(size_t)i * tiles + t];
  out[i] = (float)(sum / cells);
}

template <int ST, int VEC>
static void er_launch2(int mode, unsigned grid, hipStream_t st, const float* sd, size_t ld_d, const long long* rows,
                       const float* w, const float* sc, size_t ld_c, const float* tdb, size_t ld_t, int R, int T, int F,
                       int S, int runs, int run_len, int tiles, float* out, size_t ld_o, double* work) {
  if (mode == 0)
    hipLaunchKernelGGL((k_edr_err<ST, VEC, 0>), dim3(grid), dim3(ER_TILE), 0, st, sd, ld_d, rows, w, sc, ld_c, tdb, ld_t, R,
                       T, F, S, runs, run_len, tiles, out, ld_o, work);
  else
    hipLaunchKernelGGL((k_edr_err<ST, VEC, 1>), dim3(grid), dim3(ER_TILE), 0, st, sd, ld_d, rows, w, sc, ld_c, tdb, ld_t, R,
                       T, F, S, runs, run_len, tiles, out, ld_o, work);
}
template <int ST>
static void er_launch(bool vec, int mode, unsigned grid, hipStream_t st, const float* sd, size_t ld_d, const long long* rows,
                      const float* w, const float* sc, size_t ld_c, const float* tdb, size_t ld_t, int R, int T, int F,
                      int S, int runs, int run_len, int tiles, float* out, size_t ld_o, double* work) {
  if (vec)
    er_launch2<ST, 2>(mode, grid, st, sd, ld_d, rows, w, sc, ld_c, tdb, ld_t, R, T, F, S, runs, run_len, tiles, out, ld_o,
                      work);
  else
    er_launch2<ST, 1>(mode, grid, st, sd, ld_d, rows, w, sc, ld_c, tdb, ld_t, R, T, F, S, runs, run_len, tiles, out, ld_o,
                      work);
}

static int er_tiles(int F) { return (F + ER_TILE - 1) / ER_TILE; }

// bytes of ``work`` for mode 0: one float64 per receiver and tile of bins
extern "C" size_t gfdn_edr_err_work_bytes(int R, int F) {
  if (R <= 0 || F <= 0) return 0;
  return (size_t)R * er_tiles(F) * sizeof(double);
}

extern "C" int gfdn_edr_err(const float* sd_c64, int ld_d, const long long* rows, const float* w, const float* sc_c64,
                            int ld_c, const float* tdb, int ld_t, int R, int T, int F, int S, int mode, float* out,
                            int ld_o, void* work, void* stream) {
  if (!sd_c64 || !out || R <= 0 || T <= 0 || F <= 0 || S < 0 || ld_d < F) return GFDN_E_BADARG;
  if ((w == nullptr) != (sc_c64 == nullptr) || (S > 0) != (sc_c64 != nullptr)) return GFDN_E_BADARG;
  if (S > 0 && ld_c < F) return GFDN_E_BADARG;
  if (mode == 0) {
    if (!tdb || ld_t < F || !work || ((uintptr_t)work & 7)) return GFDN_E_BADARG;
  } else if (mode == 1) {
    if (ld_o < F) return GFDN_E_BADARG;
  } else {
    return GFDN_E_BADARG;
  }
  if (S > ER_MAX_S) return GFDN_E_UNSUPPORTED;
  const int tiles = er_tiles(F);
  // about ER_GRID_WGS waves in all, between ER_MIN_RUN and ER_RUN receivers per run
  int want = (ER_GRID_WGS + tiles - 1) / tiles;
  if (want > R) want = R;
  int run_len = (R + want - 1) / want;
  if (run_len < ER_MIN_RUN) run_len = R < ER_MIN_RUN ? R : ER_MIN_RUN;
  if (run_len > ER_RUN) run_len = ER_RUN;
  const int runs = (R + run_len - 1) / run_len;
  if ((long long)tiles * runs > 0x7fffffffLL) return GFDN_E_UNSUPPORTED;
  const bool vec = (((uintptr_t)sd_c64 | (uintptr_t)sc_c64) & 7) == 0;
  const unsigned grid = (unsigned)((long long)tiles * runs);
  hipStream_t st = (hipStream_t)stream;
#define ER_GO(ST)                                                                                                         \
  er_launch<ST>(vec, mode, grid, st, sd_c64, (size_t)ld_d, rows, w, sc_c64, (size_t)ld_c, tdb, (size_t)ld_t, R, T, F, S, \
                runs, run_len, tiles, out, (size_t)ld_o, (double*)work)
  if (S == 0)
    ER_GO(0);
  else if (S <= 8)
    ER_GO(8);
  else if (S <= 16)
    ER_GO(16);
  else if (S <= 24)
    ER_GO(24);
  else
    ER_GO(32);
#undef ER_GO
  GFDN_LAUNCH_CHECK();
  if (mode == 0) {
    hipLaunchKernelGGL(k_edr_err_sum, dim3((R + 255) / 256), dim3(256), 0, st, (const double*)work, R, tiles,
                       (double)T * (double)F, out);
    GFDN_LAUNCH_CHECK();
  }
  return 0;
}
