// Spatial render of the directional bands for gfx950: every receiver's ambisonic or directional RIR from the bands' filtered
// group signals, the ambisonic mix and the conversion to directions fused in one kernel.
//
// reference: inference.py:676-881 (``infer_all_octave_bands_directional_fdn``) with InferDiffDirectionalFDN.get_model_output
// (:402-481): per band and receiver get_response (irfft), the cut to edc_len_samps (:479-481), the optional conversion with
// the analysis matrix (:387-400), fftconvolve(.., 'same') with the band's reconstructing FIR (:807-810), the sum over the
// bands per receiver (:837-862).  None of the transforms depends on the receiver, which enters only through its
// G x (order+1)^2 spherical-harmonic weights per band:
//     ambi[i][l] = sum_{s < S} w[(i S + s) Ls + l] c[s Ls + l],       s = band G + g,  c[s Ls + l] = same_conv(irfft(..)[:L], taps)
//     out[i][j]  = sum_{l < Ls} a[j Ls + l] ambi[i][l]                (a != NULL)      or      out[i][l] = ambi[i][l]
// The ambisonic values of a receiver live in registers only: in the directional mode they never reach memory.
//
// Tiling: the register variant.  A 256-thread workgroup owns a tile of DR_TILE = 256 samples, ONE SAMPLE PER LANE, and a run
// of receivers.  It loads its tile of all S Ls signals into registers once (ST x LS VGPRs, indexed by unrolled loops only;
// ST: S rounded up to the next instantiated size, rows s >= S hold zeros and meet a repeated weight) and walks its
// receivers: per receiver S Ls FMAs into LS accumulators, then J Ls FMAs and J four-byte stores per lane.  The receiver is
// the same for the whole workgroup, so its S Ls weights and the J Ls entries of a are wave-uniform (scalar loads, an SGPR
// operand per FMA).  At the config-4 shape (Ls = 9, S = 21) the tile is 189 VGPRs and the kernel runs at two waves per SIMD
// (<= 256 VGPRs).  Why registers and not a 128-sample tile in LDS: every FMA of the inner sum takes one tile value, and
// from LDS that is one ds_read_b32 lane-dword per FMA, 128 B/clk/CU against the 64 lanes/clk (256 B/clk) the four SIMDs
// retire -- the LDS pipe would halve the FMA rate unless receivers were blocked in registers as well, which costs the
// registers the tile frees.  From registers the operand is free.  Two waves per SIMD hide little latency, but the loop
// has none to hide but its scalar loads: the tile is loaded once per run, the stores are fire-and-forget.
// One sample per lane makes every access a 4-byte one, coalesced (a wave moves 256 contiguous bytes per instruction): no
// alignment requirement on c, out or the pitches, hence no separate unaligned form.
//
// Shapes the tile does not fit (S Ls above 216 registers: S > 24 at Ls = 9, S > 13 at Ls = 16) and channel counts other
// than 1, 4, 9, 16 run the STREAMED form of the same body: the same FMAs in the same order, the tile value read from
// memory (L2) for every receiver instead of from a register.  Same bits, slower; no trained model of the project has such
// a shape (order <= 2 and <= 24 band-groups is the reference's range).
//
// Rounding: acc_l = 0, acc_l = fma(w, c, acc_l) for s = 0 .. S-1; d = 0, d = fma(a_jl, acc_l, d) for l = 0 .. Ls-1.  A
// receiver's bits do not depend on the run it falls in nor on the other receivers of the launch (the callers' rows /
// chunk arguments rely on it).
//
// Receiver split: as csrc/render.hip -- about DR_GRID_WGS workgroups, the run the fastest-varying part of the workgroup
// index so that the workgroups sharing a tile of c are dispatched back to back, never fewer than DR_MIN_RUN receivers per
// run.  At R = 838, n = 64 000 (250 tiles): 8 runs of 105 receivers; a run re-reads 189 x 4 bytes per sample against the
// 105 x 48 it writes (15 %), from L2 / Infinity Cache (c is 48 MB).
//
// A partial last tile runs the guarded form: load addresses clamped to the row's last sample, stores guarded.  Plain
// vector stores only, nothing behind sample n - 1 of any row.
#include "common.h"

#define DR_THREADS 256
#define DR_TILE DR_THREADS
#define DR_MAX_S 32
#define DR_MAX_LS 16
#define DR_MAX_J 32
#define DR_GRID_WGS 2048
#define DR_MIN_RUN 8

// ST > 0: the tile in registers, Ls == LS, SLO < S <= ST.  ST = 0: streamed, Ls <= LS.
// Every address is a wave-uniform row base (SGPRs) plus the lane's sample: one 32-bit offset register for all rows.
template <int LS, int ST, int SLO, bool DIR, bool FULL>
__device__ __forceinline__ void dr_body(const float* __restrict__ w, const float* __restrict__ c, size_t ld_c,
                                        const float* __restrict__ a, int S, int Ls, int J, int n, int r0, int r1,
                                        float* __restrict__ out, size_t ld_out, long long tile0) {
  constexpr bool HOLD = ST > 0;
  const unsigned lane = threadIdx.x;
  const bool live = FULL || tile0 + lane < n;
  const unsigned ll = live ? lane : (unsigned)(n - 1 - tile0);       // (clamped: the value is never stored)
  const int ls = HOLD ? LS : Ls;
  c += tile0;
  out += tile0;
  float cr[HOLD ? ST * LS : 1];
  if (HOLD) {
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      // (rows s >= S: a valid row is loaded and dropped -- a branch around the load would serialise the loads)
      const bool real = s < SLO || s < S;
#pragma unroll
      for (int l = 0; l < LS; ++l) {
        const float v = (c + (size_t)((real ? s : S - 1) * LS + l) * ld_c)[ll];
        cr[s * LS + l] = real ? v : 0.f;
      }
    }
  }
  for (int i = r0; i < r1; ++i) {
    const float* __restrict__ wi = w + (size_t)i * S * ls;
    float acc[LS];
#pragma unroll
    for (int l = 0; l < LS; ++l) acc[l] = 0.f;
    if (HOLD) {
#pragma unroll
      for (int s = 0; s < ST; ++s) {
        const int sw = (s < SLO || s < S) ? s : S - 1;               // (behind S: the last weights again, on a zero row)
#pragma unroll
        for (int l = 0; l < LS; ++l) acc[l] = __builtin_fmaf(wi[sw * LS + l], cr[s * LS + l], acc[l]);
      }
    } else {
      const float* cs = c;
      for (int s = 0; s < S; ++s, wi += ls, cs += (size_t)ls * ld_c) {
#pragma unroll
        for (int l = 0; l < LS; ++l)
          if (l < ls) acc[l] = __builtin_fmaf(wi[l], (cs + (size_t)l * ld_c)[ll], acc[l]);
      }
    }
    if (DIR) {
      float* oj = out + (size_t)i * J * ld_out;
      const float* __restrict__ aj = a;
#pragma clang loop vectorize(disable) unroll_count(2)
      for (int j = 0; j < J; ++j, aj += ls, oj += ld_out) {
        float d = 0.f;
#pragma unroll
        for (int l = 0; l < LS; ++l)
          if (HOLD || l < ls) d = __builtin_fmaf(aj[l], acc[l], d);
        if (live) oj[lane] = d;
      }
    } else {
      float* ol = out + (size_t)i * ls * ld_out;
#pragma unroll
      for (int l = 0; l < LS; ++l)
        if ((HOLD || l < ls) && live) (ol + (size_t)l * ld_out)[lane] = acc[l];
    }
  }
}

// grid: tiles x runs workgroups, the run fastest.  Two waves per SIMD: 256 VGPRs, which the Ls = 9, S <= 24 tile fits.
template <int LS, int ST, int SLO, bool DIR>
__global__ __launch_bounds__(DR_THREADS, 2) void k_dir_render(const float* __restrict__ w, const float* __restrict__ c,
                                                           size_t ld_c, const float* __restrict__ a, int R, int S, int Ls,
                                                           int J, int n, int runs, int run_len, float* __restrict__ out,
                                                           size_t ld_out) {
  const int run = blockIdx.x % runs;
  const long long tile0 = (long long)(blockIdx.x / runs) * DR_TILE;
  const int r0 = run * run_len;
  const int r1 = r0 + run_len < R ? r0 + run_len : R;
  if (tile0 + DR_TILE <= n)
    dr_body<LS, ST, SLO, DIR, true>(w, c, ld_c, a, S, Ls, J, n, r0, r1, out, ld_out, tile0);
  else
    dr_body<LS, ST, SLO, DIR, false>(w, c, ld_c, a, S, Ls, J, n, r0, r1, out, ld_out, tile0);
}

struct DrArgs {
  const float* w;
  const float* c;
  size_t ld_c;
  const float* a;
  int R, S, Ls, J, n, runs, run_len;
  float* out;
  size_t ld_out;
  unsigned grid;
  hipStream_t st;
};

template <int LS, int ST, int SLO>
static void dr_launch(const DrArgs& g) {
  if (g.a)
    hipLaunchKernelGGL((k_dir_render<LS, ST, SLO, true>), dim3(g.grid), dim3(DR_THREADS), 0, g.st, g.w, g.c, g.ld_c, g.a, g.R,
                       g.S, g.Ls, g.J, g.n, g.runs, g.run_len, g.out, g.ld_out);
  else
    hipLaunchKernelGGL((k_dir_render<LS, ST, SLO, false>), dim3(g.grid), dim3(DR_THREADS), 0, g.st, g.w, g.c, g.ld_c, g.a, g.R,
                       g.S, g.Ls, g.J, g.n, g.runs, g.run_len, g.out, g.ld_out);
}

extern "C" int gfdn_dir_render(const float* w, const float* c, int ld_c, const float* a, int R, int S, int Ls, int J, int n,
                               float* out, int ld_out, void* stream) {
  if (!w || !c || !out || R <= 0 || S <= 0 || Ls <= 0 || n <= 0 || ld_c < n || ld_out < n || (a && J <= 0))
    return GFDN_E_BADARG;
  if (S > DR_MAX_S || Ls > DR_MAX_LS || (a && J > DR_MAX_J)) return GFDN_E_UNSUPPORTED;
  const long long tiles = ((long long)n + DR_TILE - 1) / DR_TILE;
  // about DR_GRID_WGS workgroups in all, DR_MIN_RUN receivers per run at the least
  long long want = (DR_GRID_WGS + tiles - 1) / tiles;
  if (want > R) want = R;
  int run_len = (int)((R + want - 1) / want);
  if (run_len < DR_MIN_RUN) run_len = R < DR_MIN_RUN ? R : DR_MIN_RUN;
  const int runs = (R + run_len - 1) / run_len;
  if (tiles * runs > 0x7fffffffLL) return GFDN_E_UNSUPPORTED;
  const DrArgs g{w, c, (size_t)ld_c, a, R, S, Ls, a ? J : 0, n, runs, run_len, out, (size_t)ld_out, (unsigned)(tiles * runs),
                 (hipStream_t)stream};
  // the register tile: ST x LS <= 216 values
  if (Ls == 1) {
    dr_launch<1, 32, 0>(g);
  } else if (Ls == 4) {
    if (S <= 8) dr_launch<4, 8, 0>(g);
    else if (S <= 16) dr_launch<4, 16, 8>(g);
    else dr_launch<4, 32, 16>(g);
  } else if (Ls == 9 && S <= 24) {
    if (S <= 8) dr_launch<9, 8, 0>(g);
    else if (S <= 16) dr_launch<9, 16, 8>(g);
    else if (S <= 21) dr_launch<9, 21, 16>(g);
    else dr_launch<9, 24, 21>(g);
  } else if (Ls == 16 && S <= 13) {
    if (S <= 4) dr_launch<16, 4, 0>(g);
    else if (S <= 8) dr_launch<16, 8, 4>(g);
    else dr_launch<16, 13, 8>(g);
  } else if (Ls <= 4) {                                    // streamed
    dr_launch<4, 0, 0>(g);
  } else if (Ls <= 9) {
    dr_launch<9, 0, 0>(g);
  } else {
    dr_launch<16, 0, 0>(g);
  }
  GFDN_LAUNCH_CHECK();
  return 0;
}
