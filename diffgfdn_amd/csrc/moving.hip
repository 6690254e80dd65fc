// A listener moving through a band bank's render for gfx950: the interpolated filters and the overlap-add in two launches.
//
// reference: sound_examples.py:163-226 ``dynamic_rendering_moving_receiver.filter_overlap_add``.  It walks a list of receiver
// positions one update interval of h samples at a time: f_0 = r_0, f_k = alpha r_k + (1 - alpha) f_{k-1} (:189-193, the
// recursion runs on the INTERPOLATED filter), s_k = fftconvolve(x_k, f_k, 'full') cut at the end of the output (:195-203),
// and out[k h + i] += s_k[i], where for k >= 1 the first Fd samples are t_{k-1}[i] fade_out[i] + s_k[i] fade_in[i] with
// t_{k-1} the LAST Fd samples of the cut s_{k-1} (:205-224).  Transform, interpolation and the bank's composition
// r = D[row] + sum_s W[s] C_s (render.hip) are linear, so with n = 2^p >= h + Lr - 1 and F = n / 2 + 1 bins
//     Z[k][f] = ema_k[f] X^_k[f],   ema_k = alpha R^_k + (1 - alpha) ema_{k-1},   R^_k[f] = D^[rows[k]][f] + sum_s W[k][s] C^_s[f]
// is the spectrum of s_k: neither the composed RIRs, nor the interpolated filters, nor their spectra are stored.
//
// k_moving_compose.  One bin per lane (complex64: an 8-byte access, a wave moves 512 contiguous bytes; F is odd, so rows of
// F bins start on 8-byte boundaries only), 256 lanes per workgroup.  A lane loads its bin of the S group spectra ONCE
// (ST x 2 VGPRs, ST = S rounded up to 8 / 16 / 24 / 32 as in render.hip: static indices, rows s >= S are zero and meet the
// last weight again; ST = 0: d^ already is the RIR's spectrum) and walks the segments of the chunk IN ORDER -- the
// recursion is serial in k and independent in f.  The segment is the same for the whole workgroup, so W[k][:] and rows[k]
// are scalar loads.  acc = d^, one fma per signal on the real and the imaginary part, s ascending; ema = fma(alpha, acc,
// (1 - alpha) ema); Z = ema x^.  The state ema (F) is read at the start and written at the end of the launch, by the lane
// that owns the bin: a path goes through in chunks of segments with the bits of one launch.  The loop is unrolled by four,
// which puts the loads of four segments in flight ahead of the serial update.
//
// k_moving_ola.  Gather form, no atomics: a lane owns four consecutive output samples (one when the rows do not allow a
// 16-byte access), loads them, adds the chunk's segments that cover them in ascending k -- ONE running sum from the loaded
// value on, so that a path in chunks adds in the order of a single launch and gives its bits -- and stores them.  Segment k
// covers [k h, k h + len_k), len_k = min(h + Lr - 1, P h - k h) >= h >= Fd.  On its first Fd samples (k >= 1) the term is
// t fade_out + s fade_in with fade_in[i] = i / (Fd - 1) (0.5 (1 + linspace(-1, 1, Fd)); Fd = 1: 0) and fade_out = 1 - fade_in;
// t comes from row k - 1 of the chunk or, for the chunk's first segment, from tail_in -- the last Fd samples of the cut
// last segment of the chunk before, which that launch wrote to ITS tail_out (two buffers: nothing is read and written in
// one launch).  16-byte accesses need h, the pitch and k0 h multiples of four and 16-byte aligned bases; a vector never
// straddles a segment's start then, its samples behind len_k or Fd are handled per component, and every load stays inside
// its row (index < h + Lr - 1 rounded up to four <= pitch).  Plain vector stores only.
#include "common.h"

#define MV_THREADS 256
#define MV_MAX_S 32

typedef float mv_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float2 mv_ld(const float* __restrict__ p, int f) {
  return *reinterpret_cast<const float2*>(p + 2 * (size_t)f);
}

// grid: ceil(F / MV_THREADS) workgroups.  Pitches in complex elements.
template <int ST, bool ROWS>
__global__ __launch_bounds__(MV_THREADS) void k_moving_compose(const float* __restrict__ dh, size_t ld_d,
                                                              const long long* __restrict__ rows,
                                                              const float* __restrict__ w, const float* __restrict__ ch,
                                                              size_t ld_c, const float* __restrict__ xh, size_t ld_x,
                                                              int nseg, int F, int S, float alpha, float oma, int first,
                                                              float* __restrict__ ema, float* __restrict__ z, size_t ld_z) {
  const int f = blockIdx.x * MV_THREADS + (int)threadIdx.x;
  if (f >= F) return;
  float2 cr[ST > 0 ? ST : 1];
  if (ST > 0) {
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      // (rows s >= S: a valid row is loaded and dropped, as in render.hip)
      const float2 v = mv_ld(ch + 2 * (size_t)(s < ST - 8 || s < S ? s : S - 1) * ld_c, f);
      cr[s] = (s < ST - 8 || s < S) ? v : make_float2(0.f, 0.f);
    }
  }
  float2 e = first ? make_float2(0.f, 0.f) : mv_ld(ema, f);
#pragma unroll 4
  for (int k = 0; k < nseg; ++k) {
    const size_t row = ROWS ? (size_t)rows[k] : (size_t)k;
    float2 acc = mv_ld(dh + 2 * row * ld_d, f);
    const float2 xv = mv_ld(xh + 2 * (size_t)k * ld_x, f);
    if (ST > 0) {
      const float* __restrict__ wk = w + (size_t)k * S;
#pragma unroll
      for (int s = 0; s < ST; ++s) {
        const float ws = wk[s < ST - 8 ? s : (s < S ? s : S - 1)];
        acc.x = __builtin_fmaf(ws, cr[s].x, acc.x);
        acc.y = __builtin_fmaf(ws, cr[s].y, acc.y);
      }
    }
    if (first && k == 0) {
      e = acc;                                                      // f_0 = r_0
    } else {
      e.x = __builtin_fmaf(alpha, acc.x, oma * e.x);
      e.y = __builtin_fmaf(alpha, acc.y, oma * e.y);
    }
    // (the product with its roundings spelled out: every copy of the unrolled loop makes the same ones)
    const float2 zv = make_float2(__builtin_fmaf(e.x, xv.x, -(e.y * xv.y)), __builtin_fmaf(e.x, xv.y, e.y * xv.x));
    *reinterpret_cast<float2*>(z + 2 * ((size_t)k * ld_z + (size_t)f)) = zv;
  }
  *reinterpret_cast<float2*>(ema + 2 * (size_t)f) = e;
}

template <int ST>
static void mv_launch(unsigned grid, hipStream_t st, const float* dh, size_t ld_d, const long long* rows, const float* w,
                      const float* ch, size_t ld_c, const float* xh, size_t ld_x, int nseg, int F, int S, float alpha,
                      int first, float* ema, float* z, size_t ld_z) {
  const float oma = 1.0f - alpha;
  if (rows)
    hipLaunchKernelGGL((k_moving_compose<ST, true>), dim3(grid), dim3(MV_THREADS), 0, st, dh, ld_d, rows, w, ch, ld_c, xh,
                       ld_x, nseg, F, S, alpha, oma, first, ema, z, ld_z);
  else
    hipLaunchKernelGGL((k_moving_compose<ST, false>), dim3(grid), dim3(MV_THREADS), 0, st, dh, ld_d, rows, w, ch, ld_c, xh,
                       ld_x, nseg, F, S, alpha, oma, first, ema, z, ld_z);
}

extern "C" int gfdn_moving_compose(const float* dh_c64, int ld_d, const long long* rows, const float* w,
                                   const float* ch_c64, int ld_c, const float* xh_c64, int ld_x, int nseg, int F, int S,
                                   float alpha, int first, float* ema_c64, float* z_c64, int ld_z, void* stream) {
  if (!dh_c64 || !xh_c64 || !ema_c64 || !z_c64 || nseg <= 0 || F <= 0 || S < 0 || ld_d < F || ld_x < F || ld_z < F)
    return GFDN_E_BADARG;
  if ((S > 0) != (w != nullptr) || (S > 0) != (ch_c64 != nullptr) || (S > 0 && ld_c < F)) return GFDN_E_BADARG;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return GFDN_E_BADARG;
  if ((((uintptr_t)dh_c64 | (uintptr_t)ch_c64 | (uintptr_t)xh_c64 | (uintptr_t)ema_c64 | (uintptr_t)z_c64) & 7) != 0)
    return GFDN_E_BADARG;                                           // (complex64 rows: one 8-byte access per bin)
  if (S > MV_MAX_S) return GFDN_E_UNSUPPORTED;
  const unsigned grid = (unsigned)((F + MV_THREADS - 1) / MV_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const size_t d = (size_t)ld_d, c = (size_t)ld_c, x = (size_t)ld_x, zz = (size_t)ld_z;
  first = first ? 1 : 0;
  if (S == 0)
    mv_launch<0>(grid, st, dh_c64, d, rows, w, ch_c64, c, xh_c64, x, nseg, F, S, alpha, first, ema_c64, z_c64, zz);
  else if (S <= 8)
    mv_launch<8>(grid, st, dh_c64, d, rows, w, ch_c64, c, xh_c64, x, nseg, F, S, alpha, first, ema_c64, z_c64, zz);
  else if (S <= 16)
    mv_launch<16>(grid, st, dh_c64, d, rows, w, ch_c64, c, xh_c64, x, nseg, F, S, alpha, first, ema_c64, z_c64, zz);
  else if (S <= 24)
    mv_launch<24>(grid, st, dh_c64, d, rows, w, ch_c64, c, xh_c64, x, nseg, F, S, alpha, first, ema_c64, z_c64, zz);
  else
    mv_launch<32>(grid, st, dh_c64, d, rows, w, ch_c64, c, xh_c64, x, nseg, F, S, alpha, first, ema_c64, z_c64, zz);
  GFDN_LAUNCH_CHECK();
  return 0;
}

// grid: ceil(span / (VEC MV_THREADS)) workgroups over the output samples [k0 h, k0 h + span) that the chunk's segments cover.
// lfull = h + Lr - 1, total = P h.  The lanes j < Fd of the launch also move the tail of the chunk's last segment.
template <int VEC>
__global__ __launch_bounds__(MV_THREADS) void k_moving_ola(const float* __restrict__ s, size_t ld_s, int nseg, int k0,
                                                          long long total, int h, int lfull, int Fd, float inv_fd1,
                                                          const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                          float* __restrict__ out, long long span) {
  const long long j0 = ((long long)blockIdx.x * MV_THREADS + (long long)threadIdx.x) * VEC;
  // the tail for the chunk behind this one: the last Fd samples of the cut last segment (len >= h >= Fd)
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    if (j0 + j < Fd) {
      const int kl = k0 + nseg - 1;
      const long long room = total - (long long)kl * h;
      const int len = room < lfull ? (int)room : lfull;
      tail_out[j0 + j] = s[(size_t)(nseg - 1) * ld_s + (size_t)(len - Fd) + (size_t)(j0 + j)];
    }
  }
  if (j0 >= span) return;
  const long long m0 = (long long)k0 * h + j0;                      // (VEC = 4: m0, span and total are multiples of four)
  float acc[VEC];
  if (VEC == 4) {
    const mv_f4 v = *reinterpret_cast<const mv_f4*>(out + m0);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = v[j];
  } else {
    acc[0] = out[m0];
  }
  // the segments k0 <= k < k0 + nseg with k h <= m0 < k h + lfull (the cut at ``total`` never bites: m0 < total)
  const long long klo_g = m0 >= lfull ? (m0 - lfull) / h + 1 : 0;
  const long long khi_g = m0 / h;
  const int klo = klo_g > k0 ? (int)klo_g : k0;
  const int khi = khi_g < k0 + nseg - 1 ? (int)khi_g : k0 + nseg - 1;
#pragma unroll 4
  for (int k = klo; k <= khi; ++k) {
    const int i0 = (int)(m0 - (long long)k * h);                    // 0 <= i0 < lfull
    const float* __restrict__ sk = s + (size_t)(k - k0) * ld_s;
    float v[VEC];
    if (VEC == 4) {
      const mv_f4 q = *reinterpret_cast<const mv_f4*>(sk + i0);     // (i0 a multiple of four: i0 + 3 < the pitch)
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[j] = q[j];
    } else {
      v[0] = sk[i0];
    }
    if (k >= 1 && i0 < Fd) {
      // the cross-fade with the tail of segment k - 1 (sound_examples.py:205-210)
      const long long roomp = total - (long long)(k - 1) * h;
      const int lenp = roomp < lfull ? (int)roomp : lfull;
      const float* __restrict__ tp = k > k0 ? sk - ld_s + (lenp - Fd) : tail_in;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int i = i0 + j;
        if (i < Fd) {
          const float fi = (float)i * inv_fd1;
          v[j] = __builtin_fmaf(tp[i], 1.0f - fi, v[j] * fi);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (i0 + j < lfull) acc[j] += v[j];
  }
  if (VEC == 4) {
    *reinterpret_cast<mv_f4*>(out + m0) = (mv_f4){acc[0], acc[1], acc[2], acc[3]};
  } else {
    out[m0] = acc[0];
  }
}

extern "C" int gfdn_moving_ola(const float* s, int ld_s, int nseg, int k0, int P, int h, int Lr, int Fd,
                               const float* tail_in, float* tail_out, float* out, void* stream) {
  if (!s || !tail_out || !out || nseg <= 0 || k0 < 0 || P <= 0 || h <= 0 || Lr <= 0 || Fd < 1 || Fd > h)
    return GFDN_E_BADARG;
  if ((long long)k0 + nseg > P) return GFDN_E_BADARG;
  if (k0 > 0 && !tail_in) return GFDN_E_BADARG;
  if (tail_in == tail_out) return GFDN_E_BADARG;                    // (read and written in one launch: two buffers)
  const long long total = (long long)P * h, lfull = (long long)h + Lr - 1;
  if (total > 0x7fffffffLL || lfull > 0x7fffffffLL || ld_s < lfull) return GFDN_E_BADARG;
  const long long start = (long long)k0 * h;
  long long end = (long long)(k0 + nseg - 1) * h + lfull;
  if (end > total) end = total;
  const long long span = end - start;                               // >= h >= Fd
  const bool vec = (((uintptr_t)s | (uintptr_t)out) & 15) == 0 && ((ld_s | h) & 3) == 0;
  const float inv_fd1 = Fd > 1 ? 1.0f / (float)(Fd - 1) : 0.0f;
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    // (h a multiple of four: so are total, start and every segment's start; span is rounded up inside ``total``)
    const long long span4 = (span + 3) / 4 * 4;
    const unsigned grid = (unsigned)((span4 / 4 + MV_THREADS - 1) / MV_THREADS);
    hipLaunchKernelGGL((k_moving_ola<4>), dim3(grid), dim3(MV_THREADS), 0, st, s, (size_t)ld_s, nseg, k0, total, h,
                       (int)lfull, Fd, inv_fd1, tail_in, tail_out, out, span4);
  } else {
    const unsigned grid = (unsigned)((span + MV_THREADS - 1) / MV_THREADS);
    hipLaunchKernelGGL((k_moving_ola<1>), dim3(grid), dim3(MV_THREADS), 0, st, s, (size_t)ld_s, nseg, k0, total, h,
                       (int)lfull, Fd, inv_fd1, tail_in, tail_out, out, span);
  }
  GFDN_LAUNCH_CHECK();
  return 0;
}
