// A moving, head-turning listener heard binaurally from the directional bands for gfx950: the binaural room transfer
// functions of a chunk of path segments in one launch, and the two-ear overlap-add with the square-root cross-fade.
//
// reference: sound_examples.py:356-535 ``binaural_dynamic_rendering`` (get_binaural_rir :425-472, binaural_filter_overlap_add
// :474-535).  Per update interval k of h samples, with nb = 2^ceil(log2 L), Kb = nb / 2 + 1, A_k (Ls, Kb) the spectrum of the
// ambisonic RIR of the position, R_k (Ls, Ls) the real SH rotation matrix of the head orientation, Hh (Ls, 2, Kb) the
// spectra of the SH-domain HRIRs:
//     Rw_0 = R_0,  Rw_k = alpha R_k + (1 - alpha) R_{k-1};   Aw_0 = A_0,  Aw_k = alpha A_k + (1 - alpha) A_{k-1}
//     B_k[e][f] = sum_n conj(Hh[n][e][f]) sum_m Rw_k[n][m] Aw_k[m][f]
// NO recursion: the interpolation takes the RAW previous position (:450-461, 470-471), unlike the omnidirectional render
// (moving.hip), whose recursion runs on the filter.  The HRTFs enter conjugated (:466).  The BRIR is irfft(B_k, nb): a
// circular product at nb.
//
// k_binaural_compose.  With the rows of the directional bands (dirrender.hip) A_k[m] = sum_s W[row_k][s][m] C^[s Ls + m], the
// path's ambisonic RIRs and their spectra never exist (bank mode); rows mode reads A_k[m] from a store of spectra instead.
// Both interpolations are linear, so they are taken on what the lane holds anyway:
//     a_k[m]    = sum_s W[row_k][s][m] C^[s Ls + m][f]   (or the store's row)          raw, S complex fmas
//     g_k[m][e] = sum_n R_k[n][m] conj(Hh[n][e][f])                                     raw, Ls complex fmas per ear
//     aw = alpha a_k + (1 - alpha) a_{k-1},  gw[e] = alpha g_k[e] + (1 - alpha) g_{k-1}[e]        (k = 0: the raw values)
//     B_k[e] += gw[e] aw                                                                 for m = 0 .. Ls - 1
// A lane owns one bin (complex64, an 8-byte access; Kb is odd, so rows start on 8-byte boundaries only), a 256-thread
// workgroup owns 256 bins and a tile of T consecutive segments.  Channel m is the OUTER loop: the lane holds the S spectra
// of channel m (ST x 2 VGPRs, ST = S rounded up to 8 / 16 / 24 / 32: static indices, rows s >= S are zero and meet the last
// weight again, as in moving.hip), its bin of the 2 Ls HRTFs (conjugated once, 4 LS VGPRs) and the tile's two-ear
// accumulators (4 T VGPRs); the raw values of segment k - 1 are carried from one segment of the tile to the next, the tile's
// first segment forms those of k - 1 itself -- by the same instructions, so a segment's bits do not depend on the tile or
// the chunk it falls in: a path in chunks gives the bits of one launch and there is no state buffer.  The segment is the
// same for the whole workgroup: its weights, its rotation matrix and its row are scalar loads.  C^ (S Ls rows) is read once
// per segment tile; the tile index is the fastest-varying part of the workgroup index, so the tiles of one bin range are
// dispatched back to back and share it in L2.  T = 16 (Ls <= 9) or 8: about 180 VGPRs, two waves per SIMD.
//
// k_binaural_ola.  moving.hip's gather form for two ears, no atomics: a lane owns ONE output sample of both ears (an 8-byte
// access to the interleaved (total, 2) output), loads it, adds the chunk's segments that cover it in ascending k -- one
// running sum from the loaded value on, so that chunks add in the order of a single launch -- and stores it.  Segment k
// covers [k h, k h + len_k), len_k = min(h + nb - 1, P h - k h) >= h >= Fd.  On its first Fd samples (k >= 1) the term is
// t fade_out + s fade_in, fade_in[i] = sqrt(i / (Fd - 1)), fade_out[i] = sqrt((Fd - 1 - i) / (Fd - 1)) (the reference's
// uncorrelated fades sqrt(0.5 (1 +- linspace(-1, 1, Fd))); Fd = 1: 0 and 1); t = the last Fd samples of the cut segment
// k - 1, from row k - 1 of the chunk or, for the chunk's first segment, from tail_in (Fd, 2), which the launch before wrote
// to ITS tail_out.  The segments' rows are read four bytes per lane, coalesced: no alignment requirement on them.
// Plain vector loads and stores only.
#include "common.h"

#define BN_THREADS 256
#define BN_MAX_S 32
#define BN_MAX_LS 16

__device__ __forceinline__ float2 bn_ld(const float* __restrict__ p, size_t row, size_t ld, int f) {
  return *reinterpret_cast<const float2*>(p + 2 * (row * ld + (size_t)f));
}

struct BnArgs {
  const float* w;            // bank mode: (rows, S, Ls) weights
  const float* ch;           // bank mode: (S Ls, ld_c) spectra
  size_t ld_c;
  const float* ah;           // rows mode: (rows, Ls, ld_a) spectra
  size_t ld_a;
  const long long* path;     // row of segment k: (path ? path[k] : k) - row_off
  long long row_off;
  const float* rot;          // (P, Ls, Ls)
  const float* hh;           // (Ls 2, ld_h)
  size_t ld_h;
  int k0, nseg, Kb, S, Ls;
  float alpha, oma;
  float* b;                  // (nseg 2, ld_b)
  size_t ld_b;
  int ktiles;
};

// the raw values of segment k for channel m: a = A_k[m][f], g[e] = sum_n R_k[n][m] conj(Hh[n][e][f])
template <int LS, int ST>
__device__ __forceinline__ void bn_raw(const BnArgs& q, int k, int m, int f, const float2 (&cr)[ST > 0 ? ST : 1],
                                       const float2 (&hc)[LS][2], float2& a, float2 (&g)[2]) {
  const size_t row = (size_t)((q.path ? q.path[k] : (long long)k) - q.row_off);
  if (ST > 0) {
    const float* __restrict__ wk = q.w + row * (size_t)q.S * q.Ls + m;
    a = make_float2(0.f, 0.f);
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      const float ws = wk[(size_t)(s < ST - 8 ? s : (s < q.S ? s : q.S - 1)) * q.Ls];
      a.x = __builtin_fmaf(ws, cr[s].x, a.x);
      a.y = __builtin_fmaf(ws, cr[s].y, a.y);
    }
  } else {
    a = bn_ld(q.ah, row * q.Ls + m, q.ld_a, f);
  }
  const float* __restrict__ rk = q.rot + (size_t)k * q.Ls * q.Ls + m;
  g[0] = g[1] = make_float2(0.f, 0.f);
#pragma unroll
  for (int n = 0; n < LS; ++n) {
    // (rows n >= Ls: a valid entry of the matrix on a zero HRTF)
    const float r = rk[(size_t)(n < q.Ls ? n : q.Ls - 1) * q.Ls];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      g[e].x = __builtin_fmaf(r, hc[n][e].x, g[e].x);
      g[e].y = __builtin_fmaf(r, hc[n][e].y, g[e].y);
    }
  }
}

// grid: ceil(Kb / BN_THREADS) x ktiles workgroups, the segment tile fastest.  ST = 0: rows mode.  Ls <= LS.
template <int LS, int ST, int T>
__global__ __launch_bounds__(BN_THREADS, 2) void k_binaural_compose(const BnArgs q) {
  const int kt = blockIdx.x % q.ktiles;
  const int f = (blockIdx.x / q.ktiles) * BN_THREADS + (int)threadIdx.x;
  if (f >= q.Kb) return;
  const int Ls = q.Ls;
  float2 hc[LS][2];
#pragma unroll
  for (int n = 0; n < LS; ++n) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float2 v = bn_ld(q.hh, (size_t)(n < Ls ? n : Ls - 1) * 2 + e, q.ld_h, f);
      hc[n][e] = n < Ls ? make_float2(v.x, -v.y) : make_float2(0.f, 0.f);      // the HRTFs enter conjugated
    }
  }
  const int ka = q.k0 + kt * T;
  const int kend = q.k0 + q.nseg;
  float2 acc[T][2];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t][0] = acc[t][1] = make_float2(0.f, 0.f);
  for (int m = 0; m < Ls; ++m) {
    float2 cr[ST > 0 ? ST : 1];
    if (ST > 0) {
#pragma unroll
      for (int s = 0; s < ST; ++s) {
        // (rows s >= S: a valid row is loaded and dropped, as in moving.hip)
        const bool real = s < ST - 8 || s < q.S;
        const float2 v = bn_ld(q.ch, (size_t)(real ? s : q.S - 1) * Ls + m, q.ld_c, f);
        cr[s] = real ? v : make_float2(0.f, 0.f);
      }
    }
    float2 ap = make_float2(0.f, 0.f), gp[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
    if (ka > 0) bn_raw<LS, ST>(q, ka - 1, m, f, cr, hc, ap, gp);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int k = ka + t;
      if (k < kend) {
        float2 a, g[2], aw, gw[2];
        bn_raw<LS, ST>(q, k, m, f, cr, hc, a, g);
        if (k == 0) {                                               // Rw_0 = R_0, Aw_0 = A_0
          aw = a;
          gw[0] = g[0];
          gw[1] = g[1];
        } else {
          aw.x = __builtin_fmaf(q.alpha, a.x, q.oma * ap.x);
          aw.y = __builtin_fmaf(q.alpha, a.y, q.oma * ap.y);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            gw[e].x = __builtin_fmaf(q.alpha, g[e].x, q.oma * gp[e].x);
            gw[e].y = __builtin_fmaf(q.alpha, g[e].y, q.oma * gp[e].y);
          }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          // acc += gw aw, every rounding spelled out: all copies of the unrolled loop make the same ones
          acc[t][e].x = __builtin_fmaf(gw[e].x, aw.x, acc[t][e].x);
          acc[t][e].x = __builtin_fmaf(-gw[e].y, aw.y, acc[t][e].x);
          acc[t][e].y = __builtin_fmaf(gw[e].x, aw.y, acc[t][e].y);
          acc[t][e].y = __builtin_fmaf(gw[e].y, aw.x, acc[t][e].y);
        }
        ap = a;
        gp[0] = g[0];
        gp[1] = g[1];
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int k = ka + t;
    if (k < kend) {
#pragma unroll
      for (int e = 0; e < 2; ++e)
        *reinterpret_cast<float2*>(q.b + 2 * (((size_t)(k - q.k0) * 2 + e) * q.ld_b + (size_t)f)) = acc[t][e];
    }
  }
}

template <int LS, int ST>
static void bn_launch(BnArgs q, hipStream_t st) {
  constexpr int T = LS <= 9 ? 16 : 8;
  q.ktiles = (q.nseg + T - 1) / T;
  const unsigned grid = (unsigned)((q.Kb + BN_THREADS - 1) / BN_THREADS) * (unsigned)q.ktiles;
  hipLaunchKernelGGL((k_binaural_compose<LS, ST, T>), dim3(grid), dim3(BN_THREADS), 0, st, q);
}

template <int LS>
static void bn_launch_s(const BnArgs& q, hipStream_t st) {
  if (q.S == 0) bn_launch<LS, 0>(q, st);
  else if (q.S <= 8) bn_launch<LS, 8>(q, st);
  else if (q.S <= 16) bn_launch<LS, 16>(q, st);
  else if (q.S <= 24) bn_launch<LS, 24>(q, st);
  else bn_launch<LS, 32>(q, st);
}

extern "C" int gfdn_binaural_compose(const float* w, const float* ch_c64, int ld_c, int S, const float* ah_c64, int ld_a,
                                     const long long* path, int row_off, int nrows, const float* rot,
                                     const float* hh_c64, int ld_h, int P, int k0, int nseg, int Kb, int Ls, float alpha,
                                     float* b_c64, int ld_b, void* stream) {
  if (!rot || !hh_c64 || !b_c64 || P <= 0 || k0 < 0 || nseg <= 0 || Kb <= 0 || Ls <= 0 || S < 0 || nrows <= 0 || row_off < 0)
    return GFDN_E_BADARG;
  if ((long long)k0 + nseg > P || ld_h < Kb || ld_b < Kb) return GFDN_E_BADARG;
  const bool bank = S > 0;
  // bank mode: w and ch and no store; rows mode: the store alone
  if (bank ? (!w || !ch_c64 || ah_c64 || ld_c < Kb) : (w || ch_c64 || !ah_c64 || ld_a < Kb)) return GFDN_E_BADARG;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return GFDN_E_BADARG;
  if ((((uintptr_t)ch_c64 | (uintptr_t)ah_c64 | (uintptr_t)hh_c64 | (uintptr_t)b_c64) & 7) != 0)
    return GFDN_E_BADARG;                                           // (complex64 rows: one 8-byte access per bin)
  if ((((uintptr_t)w | (uintptr_t)rot) & 3) != 0 || ((uintptr_t)path & 7) != 0) return GFDN_E_BADARG;
  if (!path) {
    // segment k reads row k - row_off, segment k0 - 1 included
    const long long lo = (long long)(k0 > 0 ? k0 - 1 : 0) - row_off, hi = (long long)k0 + nseg - 1 - row_off;
    if (lo < 0 || hi >= nrows) return GFDN_E_BADARG;
  }
  if (S > BN_MAX_S || Ls > BN_MAX_LS) return GFDN_E_UNSUPPORTED;
  BnArgs q{w, ch_c64, (size_t)ld_c, ah_c64, (size_t)ld_a, path, (long long)row_off, rot, hh_c64, (size_t)ld_h, k0, nseg, Kb, S,
           Ls, alpha, 1.0f - alpha, b_c64, (size_t)ld_b, 1};
  hipStream_t st = (hipStream_t)stream;
  if (Ls <= 4) bn_launch_s<4>(q, st);
  else if (Ls <= 9) bn_launch_s<9>(q, st);
  else bn_launch_s<16>(q, st);
  GFDN_LAUNCH_CHECK();
  return 0;
}

// grid: ceil(span / BN_THREADS) workgroups over the output samples [k0 h, k0 h + span) that the chunk's segments cover.
// lfull = h + nb - 1, total = P h.  Row (k - k0) 2 + e of s: ear e of segment k.  The lanes j < Fd of the launch also move
// the tail of the chunk's last segment.
__global__ __launch_bounds__(BN_THREADS) void k_binaural_ola(const float* __restrict__ s, size_t ld_s, int nseg, int k0,
                                                            long long total, int h, int lfull, int Fd, float inv_fd1,
                                                            const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                            float* __restrict__ out, long long span) {
  const long long j0 = (long long)blockIdx.x * BN_THREADS + (long long)threadIdx.x;
  if (j0 < Fd) {
    // the tail for the chunk behind this one: the last Fd samples of the cut last segment (len >= h >= Fd)
    const long long room = total - (long long)(k0 + nseg - 1) * h;
    const int len = room < lfull ? (int)room : lfull;
    const float* __restrict__ sl = s + (size_t)(nseg - 1) * 2 * ld_s + (size_t)(len - Fd) + (size_t)j0;
    *reinterpret_cast<float2*>(tail_out + 2 * j0) = make_float2(sl[0], sl[ld_s]);
  }
  if (j0 >= span) return;
  const long long m0 = (long long)k0 * h + j0;
  float2 acc = *reinterpret_cast<const float2*>(out + 2 * m0);
  // the segments k0 <= k < k0 + nseg with k h <= m0 < k h + lfull (the cut at ``total`` never bites: m0 < total)
  const long long klo_g = m0 >= lfull ? (m0 - lfull) / h + 1 : 0;
  const long long khi_g = m0 / h;
  const int klo = klo_g > k0 ? (int)klo_g : k0;
  const int khi = khi_g < k0 + nseg - 1 ? (int)khi_g : k0 + nseg - 1;
#pragma unroll 4
  for (int k = klo; k <= khi; ++k) {
    const int i0 = (int)(m0 - (long long)k * h);                    // 0 <= i0 < lfull
    const float* __restrict__ sk = s + (size_t)(k - k0) * 2 * ld_s;
    float2 v = make_float2(sk[i0], sk[ld_s + i0]);
    if (k >= 1 && i0 < Fd) {
      // the cross-fade with the tail of segment k - 1 (sound_examples.py:513-519), square-root fades
      float2 t;
      if (k > k0) {
        const long long roomp = total - (long long)(k - 1) * h;
        const int lenp = roomp < lfull ? (int)roomp : lfull;
        const float* __restrict__ tp = sk - 2 * ld_s + (lenp - Fd) + i0;
        t = make_float2(tp[0], tp[ld_s]);
      } else {
        t = *reinterpret_cast<const float2*>(tail_in + 2 * (size_t)i0);
      }
      const float fi = sqrtf((float)i0 * inv_fd1);
      const float fo = Fd > 1 ? sqrtf((float)(Fd - 1 - i0) * inv_fd1) : 1.0f;
      v.x = __builtin_fmaf(t.x, fo, v.x * fi);
      v.y = __builtin_fmaf(t.y, fo, v.y * fi);
    }
    acc.x += v.x;
    acc.y += v.y;
  }
  *reinterpret_cast<float2*>(out + 2 * m0) = acc;
}

extern "C" int gfdn_binaural_ola(const float* s, int ld_s, int nseg, int k0, int P, int h, int nb, int Fd,
                                 const float* tail_in, float* tail_out, float* out, void* stream) {
  if (!s || !tail_out || !out || nseg <= 0 || k0 < 0 || P <= 0 || h <= 0 || nb <= 0 || Fd < 1 || Fd > h)
    return GFDN_E_BADARG;
  if ((long long)k0 + nseg > P) return GFDN_E_BADARG;
  if (k0 > 0 && !tail_in) return GFDN_E_BADARG;
  if (tail_in == tail_out) return GFDN_E_BADARG;                    // (read and written in one launch: two buffers)
  const long long total = (long long)P * h, lfull = (long long)h + nb - 1;
  if (total > 0x7fffffffLL || lfull > 0x7fffffffLL || ld_s < lfull) return GFDN_E_BADARG;
  if ((((uintptr_t)out | (uintptr_t)tail_in | (uintptr_t)tail_out) & 7) != 0 || ((uintptr_t)s & 3) != 0)
    return GFDN_E_BADARG;                                           // (both ears of a sample: one 8-byte access)
  const long long start = (long long)k0 * h;
  long long end = (long long)(k0 + nseg - 1) * h + lfull;
  if (end > total) end = total;
  const long long span = end - start;                               // >= h >= Fd
  const float inv_fd1 = Fd > 1 ? 1.0f / (float)(Fd - 1) : 0.0f;
  const unsigned grid = (unsigned)((span + BN_THREADS - 1) / BN_THREADS);
  hipLaunchKernelGGL(k_binaural_ola, dim3(grid), dim3(BN_THREADS), 0, (hipStream_t)stream, s, (size_t)ld_s, nseg, k0, total,
                     h, (int)lfull, Fd, inv_fd1, tail_in, tail_out, out, span);
  GFDN_LAUNCH_CHECK();
  return 0;
}
