// The mix at a signal-to-noise ratio with the notebooks' peak rule, once, for pe_stim_finish and pe_noise_mix: piece
// sums of squares (in place: under a fade), row rms and scale, the mix with piece peaks, row peak and normalisation,
// over any row plan that a traits struct describes.  Stands on the piece geometry and the reductions of pieces.h.
#pragma once
#include <math.h>
#include "pieces.h"

namespace pe {

// What the mix reads of a row plan is a traits struct R of the plan's own file, every kernel below a template on it,
// so that a plan's instance has its fields as constants (the plan itself, `meta`, is n_rows x R::kFields int64 and
// opens with the shared row header):
//   kFields, kPieceOffset   int64 per row; the field of the row's piece prefix
//   kFade                   the field of the row's fade length; -1: the plan has none, no fade
//   kNoiseOffset            the field of the offset of the row's noise in the noise tensor, a row with -1 there having
//                           none; -1: the plan has no such field, the noise lies where the row does
//   kSnrStride              snr_db of row r is snr[r kSnrStride]
//   kInPlace                y is mixed into itself (what a fade needs); else x -> y, and x is only read
//   kPeakLaunch             the row peaks take a launch of their own (plans whose rows may have thousands of pieces)
// A row's pieces are those of its n samples, (n + kPiece - 1) / kPiece from the prefix on, whatever else the plan
// counts there.

// stats of a row, doubles: max |y| before the division, rms of the signal, rms of the noise, the scale of the noise
enum { ST_PEAK, ST_RMS_S, ST_RMS_N, ST_SCALE, ST_K };
constexpr int kPartFields = 3;                   // doubles of a piece in `part`: sum of signal^2, of noise^2, max |y|

template <class R>
__device__ __forceinline__ const float* mix_noise_of(const long* m, const float* noise) {
  if constexpr (R::kNoiseOffset < 0) return noise + m[kRowOffset];
  else return noise && m[R::kNoiseOffset] >= 0 ? noise + m[R::kNoiseOffset] : nullptr;
}

// window[i] of a row of n samples with a fade of F: ramp[i] over the head, ramp[n - 1 - i] over the tail (the tail
// overwrites the head where they overlap), ramp[j] = 0.5 - 0.5 cos(j (pi / (F - 1))) with the last angle pi itself;
// exactly 1.0 outside the fades and for F <= 0.
__device__ __forceinline__ double fade_window(long i, long n, long F) {
#pragma clang fp contract(off)
  constexpr double pi = 3.141592653589793;
  if (F <= 0) return 1.0;
  long j = -1;
  if (i < F) j = i;
  if (i >= n - F) j = n - 1 - i;
  if (j < 0) return 1.0;
  const double ang = j == 0 ? 0.0 : (j == F - 1 ? pi : (double)j * (pi / (double)(F - 1)));
  return 0.5 - 0.5 * cos(ang);
}

// float32((rms_s / 10^(snr_db / 20)) / rms_n) as a double; 0, no mix, when the signal or the noise is silent
__device__ __forceinline__ double snr_scale(double rms_s, double rms_n, double snr_db) {
#pragma clang fp contract(off)
  if (!(rms_s > 0.0 && rms_n > 0.0)) return 0.0;
  const double target = rms_s / pow(10.0, snr_db / 20.0);
  return (double)(float)(target / rms_n);
}

// max of the row's piece peaks, each a float32 (the order is immaterial); every thread gets it
template <class R>
__device__ __forceinline__ float mix_row_peak(const double* part, const long* m, float* s_red, int tid) {
  const long pieces = (m[kRowLength] + kPiece - 1) / kPiece;
  const double* pr = part + kPartFields * m[R::kPieceOffset] + 2;
  float pk = 0.f;
  for (long p = tid; p < pieces; p += kThreads) pk = fmaxf(pk, (float)pr[kPartFields * p]);
  return block_max(pk, s_red, tid);
}

namespace {   // kernels: every translation unit that includes this file owns its instances

// part[g] = {sum of signal^2, sum of noise^2, -} of the piece: a thread adds its kRun samples in order, the threads a
// tree.  In place the signal is v = float32(float64(y) window), stored back, and max |v| is the piece's peak, which
// stands for the rows that the mix then skips; else x is only read: no window, no store, no peak.
template <class R>
__global__ __launch_bounds__(kThreads) void mix_sums_kernel(const long* __restrict__ meta, int n_rows, long pieces,
                                                            const float* __restrict__ x,
                                                            const float* __restrict__ noise, float* __restrict__ y,
                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_sum[kThreads];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, R::kFields, R::kPieceOffset, g);
    const long* m = meta + (long)row * R::kFields;
    const long n = m[kRowLength], i0 = (g - m[R::kPieceOffset]) * kPiece + (long)tid * kRun;
    const float* nr = mix_noise_of<R>(m, noise);
    long F = 0;
    if constexpr (R::kFade >= 0) F = m[R::kFade];
    double ss = 0.0, sn = 0.0, pk = 0.0;
#pragma unroll
    for (int u = 0; u < kRun; ++u)
      if (i0 + u < n) {
        float val;
        if constexpr (R::kInPlace) {
          float* yr = y + m[kRowOffset];
          val = (float)((double)yr[i0 + u] * fade_window(i0 + u, n, F));
          yr[i0 + u] = val;
          pk = fmax(pk, fabs((double)val));
        } else {
          val = x[m[kRowOffset] + i0 + u];
        }
        ss += (double)val * (double)val;
        if (nr) { const double q = (double)nr[i0 + u]; sn += q * q; }
      }
    const double tss = block_sum_d(ss, s_sum, tid), tsn = block_sum_d(sn, s_sum, tid);
    const double tpk = R::kInPlace ? block_max_d(pk, s_sum, tid) : 0.0;
    if (tid == 0) { part[kPartFields * g] = tss; part[kPartFields * g + 1] = tsn; part[kPartFields * g + 2] = tpk; }
  }
}

// stats[row] = {0, rms of the signal, rms of the noise, scale}; {0, 0, 0, 0} for n == 0.  One workgroup per row:
// kThreads piece sums at a time come into LDS, thread 0 adds them in piece order.
template <class R>
__global__ __launch_bounds__(kThreads) void mix_scale_kernel(const long* __restrict__ meta,
                                                             const double* __restrict__ snr,
                                                             const double* __restrict__ part,
                                                             double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double s_s[kThreads], s_n[kThreads];
  const int tid = threadIdx.x, row = blockIdx.x;
  const long* m = meta + (long)row * R::kFields;
  const long n = m[kRowLength], pieces = (n + kPiece - 1) / kPiece;
  const double* pr = part + kPartFields * m[R::kPieceOffset];
  double ss = 0.0, sn = 0.0;
  for (long p0 = 0; p0 < pieces; p0 += kThreads) {
    const int count = (int)(pieces - p0 < kThreads ? pieces - p0 : kThreads);
    if (tid < count) { s_s[tid] = pr[kPartFields * (p0 + tid)]; s_n[tid] = pr[kPartFields * (p0 + tid) + 1]; }
    __syncthreads();
    if (tid == 0)
      for (int p = 0; p < count; ++p) { ss += s_s[p]; sn += s_n[p]; }
    __syncthreads();
  }
  if (tid != 0) return;
  const double rs = n > 0 ? sqrt(ss / (double)n) : 0.0, rn = n > 0 ? sqrt(sn / (double)n) : 0.0;
  double* st = stats + (long)row * ST_K;
  st[ST_PEAK] = 0.0; st[ST_RMS_S] = rs; st[ST_RMS_N] = rn;
  st[ST_SCALE] = snr_scale(rs, rn, snr[(long)row * R::kSnrStride]);
}

// y = x + float32(noise scale), both in float32, for a row with noise and a scale, y = x for any other, and
// part[g].peak = max |y| of the piece.  In place x is not read, y is mixed into itself, and such another row is
// skipped: the piece peak of the sums stands.
template <class R>
__global__ __launch_bounds__(kThreads) void mix_add_kernel(const long* __restrict__ meta, int n_rows, long pieces,
                                                           const float* __restrict__ x,
                                                           const float* __restrict__ noise,
                                                           const double* __restrict__ stats, float* __restrict__ y,
                                                           double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float s_red[kThreads / 64];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, R::kFields, R::kPieceOffset, g);
    const long* m = meta + (long)row * R::kFields;
    const double sc = stats[(long)row * ST_K + ST_SCALE];
    const float* nr = mix_noise_of<R>(m, noise);
    const long n = m[kRowLength], base = (g - m[R::kPieceOffset]) * kPiece;
    float* yr = y + m[kRowOffset];
    const float* xr = R::kInPlace ? yr : x + m[kRowOffset];
    const bool mixed = nr && sc != 0.0;                              // uniform over the workgroup
    if (R::kInPlace && !mixed) continue;
    const float scale = (float)sc;
    float pk = 0.f;
    for (int j = tid; j < kPiece && base + j < n; j += kThreads) {
      float val = xr[base + j];
      if (mixed) {
        const float q = nr[base + j] * scale;
        val = val + q;
      }
      yr[base + j] = val;
      pk = fmaxf(pk, fabsf(val));
    }
    pk = block_max(pk, s_red, tid);
    if (tid == 0) part[kPartFields * g + 2] = (double)pk;
  }
}

// stats[row].peak = the row's peak.  One workgroup per row: the launch of a plan with kPeakLaunch.
template <class R>
__global__ __launch_bounds__(kThreads) void mix_peak_kernel(const long* __restrict__ meta,
                                                            const double* __restrict__ part,
                                                            double* __restrict__ stats) {
  __shared__ float s_red[kThreads / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  const float pk = mix_row_peak<R>(part, meta + (long)row * R::kFields, s_red, tid);
  if (tid == 0) stats[(long)row * ST_K + ST_PEAK] = (double)pk;
}

// The notebooks' peak rule on y, a division by the float32 of a double sum.  With kPeakLaunch the row's peak is in
// stats; else every piece's workgroup finds it itself and the row's first one writes it to stats.
template <class R>
__global__ __launch_bounds__(kThreads) void mix_normalize_kernel(const long* __restrict__ meta, int n_rows,
                                                                 long pieces, const double* __restrict__ part,
                                                                 float* __restrict__ y, double* stats) {
#pragma clang fp contract(off)
  __shared__ float s_red[kThreads / 64];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, R::kFields, R::kPieceOffset, g);
    const long* m = meta + (long)row * R::kFields;
    const long n = m[kRowLength], base = (g - m[R::kPieceOffset]) * kPiece;
    if (base >= n) continue;                                         // uniform over the workgroup
    double* st = stats + (long)row * ST_K;
    double peak;
    if constexpr (R::kPeakLaunch) {
      peak = st[ST_PEAK];
    } else {
      peak = (double)mix_row_peak<R>(part, m, s_red, tid);
      if (base == 0 && tid == 0) st[ST_PEAK] = peak;
    }
    if (peak > 0.99) {
      const float d = (float)(peak + 1e-6);
      float* yr = y + m[kRowOffset];
      for (int j = tid; j < kPiece && base + j < n; j += kThreads) yr[base + j] = yr[base + j] / d;
    }
  }
}

// The launches of the mix of x and noise into y (R::kInPlace: of y and noise into y; x is not used) on `stream`:
// PE_OK, or the status of a launch that failed.  Four launches, the last one finding the row peaks as it divides; with
// R::kPeakLaunch five, the row peaks in one of their own, and four again without `divide`, which leaves y as the mix
// made it.
template <class R>
int launch_snr_mix(const long* meta, int n_rows, const double* snr, long pieces, const float* x, const float* noise,
                   float* y, bool divide, double* stats, double* part, hipStream_t stream) {
  const dim3 grid(grid_of(pieces)), rows(n_rows), wg(kThreads);
  hipLaunchKernelGGL(mix_sums_kernel<R>, grid, wg, 0, stream, meta, n_rows, pieces, x, noise, y, part);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(mix_scale_kernel<R>, rows, wg, 0, stream, meta, snr, part, stats);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(mix_add_kernel<R>, grid, wg, 0, stream, meta, n_rows, pieces, x, noise, stats, y, part);
  PE_LAUNCH_CHECK();
  if (R::kPeakLaunch) {
    hipLaunchKernelGGL(mix_peak_kernel<R>, rows, wg, 0, stream, meta, part, stats);
    PE_LAUNCH_CHECK();
    if (!divide) return PE_OK;
  }
  hipLaunchKernelGGL(mix_normalize_kernel<R>, grid, wg, 0, stream, meta, n_rows, pieces, part, y, stats);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

}  // namespace
}  // namespace pe
