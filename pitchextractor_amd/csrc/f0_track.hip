// F0 labels on the GPU: Boersma's autocorrelation method (P. Boersma, "Accurate short-term analysis of the
// fundamental frequency and the harmonics-to-noise ratio of a sampled sound", IFA Proceedings 17, 1993), the
// algorithm behind Praat's "Sound: To Pitch (ac)" and the reference's `praat` / `parselmouth` backend
// (f0_backends.py:437-593).  Pinned by the float64 restatement in tests/f0_track_ref.py; parity with Praat's own
// binary is unpinned.
//
// Ragged batches: pe_f0_track_plan (host only) derives the constants of a configuration and lays the rows out by
// prefix offsets of their frame counts; five launches then serve any batch:
//   1. stats:  pe_row_stats, for any plan (row header of dsp.h): every row in 64 pieces, one workgroup each: double
//      partial sums, added in a fixed order to the mean; then max |x - mean| per piece and per row (three launches).
//   2. frames: one workgroup per (row, frame), found by a binary search over the frame offsets.  The window is staged
//      from HBM once into LDS; local mean and peak; Hann window; the real FFT runs as a packed half-length complex
//      radix-4 Stockham FFT in place in LDS (fft_lds, dsp.h; each thread holds its butterflies' inputs in registers
//      across the barrier); power spectrum; inverse transform; r[lag] = ac[lag] / (ac[0] window_r[lag]); ordered
//      compaction of the local maxima; parabolic vertex + depth-30 sinc strength one maximum per thread; the best 14
//      by rank; depth-70 sinc refinement one candidate per 16-lane group, evaluated in double.
//   3. path:   one wave per row walks the frames (15 x 15 transitions per step); back-pointers are one byte per
//      candidate, in LDS (sized by the batch's longest row that fits) and in the caller's workspace otherwise.  This pass is a chain of
//      dependent steps: it is latency-bound by construction.
// No atomics, no cross-workgroup communication: a row's result does not depend on the batch around it.
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kCand = 15;                 // candidates per frame, [0] = unvoiced
constexpr int kThreads = 256;
constexpr int kLdsFrames = 4000;          // back-pointer rows of 16 bytes that stay in LDS (64 000 bytes)
constexpr int kDepthFirst = 30, kDepthRefine = 70;
constexpr int kRefineSteps = 4;
constexpr float kSilentRatio = 9.5367431640625e-07f;     // 2^-20

enum { T_XOFF, T_N, T_FRAMES, T_FOFF, T_BPOFF, T_K };
static_assert(T_XOFF == kRowOffset && T_N == kRowLength, "the plan opens with the shared row header");

struct TrackConsts {
  int nw, hw, nper, hper, nfft, log2c, maxlag, sr;
  double ceiling, dt;
  float min_pitch, ceil_f, silence, voicing, octave_cost, jump_c, vuv_c;
};

// step 1 of the algorithm for (sr, hop, config); config = {min_pitch, max_pitch, silence_threshold,
// voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost}
int derive(int sr, int hop, const double* cfg, TrackConsts* k) {
#pragma clang fp contract(off)
  if (!cfg || sr <= 0 || hop <= 0) return PE_E_ARG;
  for (int i = 0; i < 7; ++i)
    if (!isfinite(cfg[i])) return PE_E_ARG;
  const double minp = cfg[0], maxp = cfg[1];
  if (!(minp > 0.0) || !(minp < maxp) || !(cfg[2] > 0.0) || !(cfg[3] > 0.0) || cfg[4] < 0.0 || cfg[5] < 0.0 ||
      cfg[6] < 0.0)
    return PE_E_ARG;
  const double ceiling = maxp < 0.5 * sr ? maxp : 0.5 * sr;
  if (!(minp < ceiling)) return PE_E_ARG;
  const double w = floor(3.0 * sr / minp);
  if (w > 1e7) return PE_E_UNSUPPORTED;
  const long nw = 2 * ((long)w / 2 - 1);
  long nfft = 1;
  while ((double)nfft < 1.5 * (double)nw) nfft *= 2;
  if (nw < 16 || nfft < 1024 || nfft > 8192) return PE_E_UNSUPPORTED;
  k->nw = (int)nw;
  k->hw = (int)(nw / 2);
  k->nper = (int)floor(sr / minp);
  k->hper = k->nper / 2 + 1;
  k->nfft = (int)nfft;
  k->log2c = 0;
  while ((2 << k->log2c) < nfft) ++k->log2c;
  const int ml = (int)(nw / 3) + 2;
  k->maxlag = ml < k->hw ? ml : k->hw;
  k->sr = sr;
  k->ceiling = ceiling;
  k->dt = (double)hop / (double)sr;
  const double c = 0.01 / k->dt;
  k->min_pitch = (float)minp;
  k->ceil_f = (float)ceiling;
  k->silence = (float)cfg[2];
  k->voicing = (float)cfg[3];
  k->octave_cost = (float)cfg[4];
  k->jump_c = (float)(cfg[5] * c);
  k->vuv_c = (float)(cfg[6] * c);
  return PE_OK;
}

long table_floats(const TrackConsts& k) {     // twiddles (C float2), split roots (C + 1 float2), window, window_r
  return fft_table_floats(k.nfft / 2) + k.nw + k.hw + 1;
}

// step 2: frames and first centre of a row of n samples, in float64 in exactly this order
void frame_layout(long n, const TrackConsts& k, double minp, long* frames, double* t1) {
#pragma clang fp contract(off)
  const double duration = (double)n / (double)k.sr;
  const double span = duration - 3.0 / minp;
  const double q = span / k.dt;
  long nf = (long)floor(q) + 1;
  if (nf < 0) nf = 0;
  const double a = duration / 2.0;
  const double b = (double)nf * k.dt;
  const double c = b / 2.0;
  const double d = a - c;
  *frames = nf;
  *t1 = d + k.dt / 2.0;
}

// ---- 1. per-row statistics -------------------------------------------------------------------------------------------
// A row is cut into kChunks equal pieces (by its own length only, so the result does not depend on the batch); one
// workgroup per (row, piece).  Partial sums are doubles added in a fixed order; no atomics.  Reads the row header only.
constexpr int kChunks = 64;

__global__ __launch_bounds__(kThreads) void f0_sum_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                          int fields, double* __restrict__ part) {
  __shared__ double s_sum[kThreads];
  const int row = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const long* m = meta + (long)row * fields;
  const long n = m[kRowLength], per = (n + kChunks - 1) / kChunks;
  const long lo = c * per, hi = lo + per < n ? lo + per : n;
  const float* xr = x + m[kRowOffset];
  double s = 0.0;
  for (long i = lo + tid; i < hi; i += kThreads) s += (double)xr[i];
  s_sum[tid] = s;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_sum[tid] += s_sum[tid + h];
    __syncthreads();
  }
  if (tid == 0) part[(long)row * kChunks + c] = s_sum[0];
}

__global__ __launch_bounds__(kThreads) void f0_peak_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                           int fields, const double* __restrict__ part,
                                                           float* __restrict__ pk, float* __restrict__ stats) {
  __shared__ float s_max[kThreads];
  __shared__ float s_mean;
  const int row = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const long* m = meta + (long)row * fields;
  const long n = m[kRowLength], per = (n + kChunks - 1) / kChunks;
  const long lo = c * per, hi = lo + per < n ? lo + per : n;
  const float* xr = x + m[kRowOffset];
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < kChunks; ++k) s += part[(long)row * kChunks + k];
    s_mean = n > 0 ? (float)(s / (double)n) : 0.f;
    if (c == 0) stats[2 * row] = s_mean;
  }
  __syncthreads();
  const float mean = s_mean;
  float v = 0.f;
  for (long i = lo + tid; i < hi; i += kThreads) v = fmaxf(v, fabsf(xr[i] - mean));
  s_max[tid] = v;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_max[tid] = fmaxf(s_max[tid], s_max[tid + h]);
    __syncthreads();
  }
  if (tid == 0) pk[(long)row * kChunks + c] = s_max[0];
}

__global__ __launch_bounds__(kThreads) void f0_peak_final_kernel(const float* __restrict__ pk, int n_rows,
                                                                 float* __restrict__ stats) {
  const int row = blockIdx.x * kThreads + threadIdx.x;
  if (row >= n_rows) return;
  float v = 0.f;
  for (int k = 0; k < kChunks; ++k) v = fmaxf(v, pk[(long)row * kChunks + k]);
  stats[2 * row + 1] = v;
}

// ---- 2. frames ---------------------------------------------------------------------------------------------------------
// Sinc interpolation of the symmetric r (r[-k] = r[k], known for |k| <= hw) at x > 0 with a raised-cosine taper that
// reaches zero one sample beyond `depth` taps on either side (Praat's NUM_interpolate_sinc):
//   sum over taps at distance d of r[tap] * sin(pi d) / (pi d) * (0.5 + 0.5 cos(pi d / (d_nearest + depth))).
// sin(pi d) is +-sin(pi frac) on either side; the taper's cosine advances by a fixed angle from tap to tap, so it is
// carried as a rotation (two transcendental pairs per side instead of one per tap).  One side's taps k0, k0 + KSTEP, ..
template <int KSTEP>
__device__ __forceinline__ float sinc_side(const float* r, int il, float fr, int dep, bool right, int k0) {
  const float inv_big = __builtin_amdgcn_rcpf(fr + (float)dep);
  float c = cospif((fr + (float)k0) * inv_big), s = sinpif((fr + (float)k0) * inv_big);
  const float cd = cospif((float)KSTEP * inv_big), sd = sinpif((float)KSTEP * inv_big);
  float sgn = (k0 & 1) ? -1.f : 1.f;
  float acc = 0.f;
  for (int k = k0; k < dep; k += KSTEP) {
    int ix = right ? il + 1 + k : il - k;
    ix = ix < 0 ? -ix : ix;
    const float w = sgn * __builtin_amdgcn_rcpf(fr + (float)k) * (0.5f + 0.5f * c);
    acc = fmaf(r[ix], w, acc);
    const float cn = c * cd - s * sd;
    s = s * cd + c * sd;
    c = cn;
    if (KSTEP & 1) sgn = -sgn;
  }
  return acc;
}

// One lane does both sides: the depth-30 strengths that only rank the maxima.
__device__ __forceinline__ float sinc_interp(const float* r, int hw, float x, int depth) {
  const float fl = floorf(x);
  const int il = (int)fl;
  const float frac = x - fl;
  int dep = hw - il;
  dep = dep < depth ? dep : depth;
  if (frac == 0.f || dep <= 0) return r[il < hw ? il : hw];
  const float s0 = sinpif(frac) * (1.f / kPiF);
  return (sinc_side<1>(r, il, frac, dep, false, 0) + sinc_side<1>(r, il, 1.f - frac, dep, true, 0)) * s0;
}

// The refinement evaluates the same interpolation in double (r stays float32).  Its parabolic steps divide a
// difference of two interpolated values by their second difference, 0.5 h (y+ - y-) / (2 y0 - y- - y+) with h = 1/8
// lag at the end: on a broad peak that turns an error of one float32 rounding in the values (5e-8) into 1e-2 cents and
// more, with a spread of 15x from one realisation of the rounding to another (measured on the restatement, DESIGN.md
// section 13).  In double that term vanishes and what is left is the float32 rounding of r itself (below 1e-3 cents).
// The sixteen lanes of a group (`gl` = lane in the group) split the taps, even lanes the left side and odd lanes the
// right one, and add their parts up.
__device__ __forceinline__ double rcp_d(double d) {
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  return fma(fma(-d, y, 1.0), y, y);
}

__device__ __noinline__ double sinc_refine(const float* r, int hw, double x, int depth, int gl) {
  const double fl = floor(x);
  const int il = (int)fl;
  const double frac = x - fl;
  int dep = hw - il;
  dep = dep < depth ? dep : depth;
  if (frac == 0.0 || dep <= 0) return (double)r[il < hw ? il : hw];
  const bool right = gl & 1;
  const int k0 = gl >> 1;
  const double fr = right ? 1.0 - frac : frac;
  const double inv_big = rcp_d(fr + (double)dep);
  double s, c, sd, cd;
  sincospi((fr + (double)k0) * inv_big, &s, &c);
  sincospi(8.0 * inv_big, &sd, &cd);
  double sgn = (k0 & 1) ? -1.0 : 1.0;                    // k advances by 8: the sign of sin(pi d) stays
  double acc = 0.0;
  for (int k = k0; k < dep; k += 8) {
    int ix = right ? il + 1 + k : il - k;
    ix = ix < 0 ? -ix : ix;
    const double w = sgn * rcp_d(fr + (double)k) * (0.5 + 0.5 * c);
    acc = fma((double)r[ix], w, acc);
    const double cn = c * cd - s * sd;
    s = s * cd + c * sd;
    c = cn;
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  return acc * (sinpi(frac) * 0.31830988618379067154);
}

template <int LOG2C>
__global__ __launch_bounds__(kThreads) void f0_frames_kernel(const float* __restrict__ x,
                                                             const long* __restrict__ meta,
                                                             const double* __restrict__ t1,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ tables, int n_rows, long total,
                                                             TrackConsts K, float* __restrict__ cand_f,
                                                             float* __restrict__ cand_s, int* __restrict__ cand_n) {
  constexpr int C = 1 << LOG2C, N = 2 * C;
  constexpr int NQ = C / kThreads;                                  // bins per thread
  constexpr int NL = (N / 3 + kThreads - 1) / kThreads;             // lags per thread, hw < N / 3
  __shared__ float2 s_buf[C];
  __shared__ float s_red[4];
  __shared__ int s_cnt;
  __shared__ int s_sel[16];
  float* fb = reinterpret_cast<float*>(s_buf);
  // lists of local maxima live in the upper half of the buffer, r[0 .. hw] in the lower one (hw < N / 3)
  int* l_lag = reinterpret_cast<int*>(fb + C);
  float* l_x = fb + C + N / 8;
  float* l_s = fb + C + 2 * (N / 8);
  float* l_sc = fb + C + 3 * (N / 8);
  const float2* tw = reinterpret_cast<const float2*>(tables);
  const float2* tr = tw + C;
  const float* win = tables + fft_table_floats(C);
  const float* wr = win + K.nw;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nw = K.nw, hw = K.hw;
  const float srf = (float)K.sr;

  for (long g = blockIdx.x; g < total; g += gridDim.x) {
    const int row = find_row(meta, n_rows, T_K, T_FOFF, g);
    const long* m = meta + (long)row * T_K;
    const long n = m[T_N];
    const float* xr = x + m[T_XOFF];
    const long f = g - m[T_FOFF];
    long left0;
    {
#pragma clang fp contract(off)
      const double ft = (double)f * K.dt;
      const double t = t1[row] + ft;
      const double pos = t * (double)K.sr;
      left0 = (long)floor(pos - 0.5);
    }
    const long start0 = left0 + 1 - hw;
    const float gmean = stats[2 * row], gpeak = stats[2 * row + 1];
    float* cf = cand_f + g * kCand;
    float* cs = cand_s + g * kCand;

    for (int j = tid; j < N; j += kThreads) {
      const long idx = start0 + j;
      fb[j] = (j < nw && idx >= 0 && idx < n) ? xr[idx] - gmean : 0.f;
    }
    __syncthreads();
    float part = 0.f;
    for (int j = hw - K.nper + tid; j < hw + K.nper; j += kThreads) part += fb[j];
    const float lmean = block_sum(part, s_red, tid) / (float)(2 * K.nper);
    float pk = 0.f;
    for (int j = hw - K.hper + tid; j < hw + K.hper; j += kThreads) pk = fmaxf(pk, fabsf(fb[j] - lmean));
    const float lpeak = block_max(pk, s_red, tid);
    const bool silent = gpeak == 0.f || lpeak < kSilentRatio * gpeak;
    float intensity = gpeak > 0.f ? lpeak / gpeak : 0.f;
    intensity = intensity > 1.f ? 1.f : intensity;
    const float unvoiced = K.voicing + fmaxf(0.f, 2.f - intensity / (K.silence / (1.f + K.voicing)));
    if (silent) {                                                   // uniform over the workgroup
      if (tid < kCand) {
        cf[tid] = 0.f;
        cs[tid] = tid == 0 ? unvoiced : 0.f;
      }
      if (tid == 0) cand_n[g] = 1;
      __syncthreads();
      continue;
    }
    for (int j = tid; j < nw; j += kThreads) fb[j] = (fb[j] - lmean) * win[j];
    __syncthreads();
    fft_lds<LOG2C, false, kThreads>(s_buf, tw, tid);

    // power spectrum of the N-point real transform, bins 0 .. C
    float p[NQ], pC = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = tid + kThreads * q;
      float2 e, o;
      const float2 t = real_fft_bin(s_buf, tr[k], C, k, e, o);
      const float2 X = cadd(e, t);
      p[q] = X.x * X.x + X.y * X.y;
      if (k == 0) {                                                 // bin C: E - O
        const float2 Xc = csub(e, o);
        pC = Xc.x * Xc.x + Xc.y * Xc.y;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) fb[tid + kThreads * q] = p[q];
    if (tid == 0) fb[C] = pC;
    __syncthreads();
    // packed input of the inverse real transform of the (real, even) power spectrum
    float2 y[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = tid + kThreads * q;
      const float pk2 = fb[k], pc = fb[C - k];
      const float e = 0.5f * (pk2 + pc), hd = 0.5f * (pk2 - pc);
      const float2 w = tr[k];                                       // (cos, -sin) of 2 pi k / N
      y[q] = make_float2(e + hd * w.y, hd * w.x);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) s_buf[tid + kThreads * q] = y[q];
    __syncthreads();
    fft_lds<LOG2C, true, kThreads>(s_buf, tw, tid);

    // r[lag] = ac[lag] / (ac[0] window_r[lag]), lag 0 .. hw; the transform's scale cancels
    const float ac0 = fb[0];
    float rr[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int lag = tid + kThreads * q;
      rr[q] = (lag <= hw) ? (lag == 0 ? 1.f : fb[lag] / (ac0 * wr[lag])) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int lag = tid + kThreads * q;
      if (lag <= hw) fb[lag] = rr[q];
    }
    __syncthreads();

    // local maxima in lag order (wave 0, ballot prefix)
    if (tid < 64) {
      int cnt = 0;
      const float thr = 0.5f * K.voicing;
      for (int base = 2; base < K.maxlag; base += 64) {
        const int i = base + lane;
        bool flag = false;
        if (i < K.maxlag) {
          const float a = fb[i - 1], b = fb[i], c = fb[i + 1];
          flag = b > thr && b > a && b >= c;
        }
        const unsigned long long mask = __ballot(flag);
        if (flag) l_lag[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        cnt += __popcll(mask);
      }
      if (tid == 0) s_cnt = cnt;
    }
    __syncthreads();
    const int M = s_cnt;
    for (int mi = tid; mi < M; mi += kThreads) {
      const int i = l_lag[mi];
      const float a = fb[i - 1], b = fb[i], c = fb[i + 1];
      const float dr = 0.5f * (c - a), d2r = (2.f * b - a) - c;
      const float x0 = (float)i + dr / d2r;
      float s = sinc_interp(fb, hw, x0, kDepthFirst);
      if (s > 1.f) s = 1.f / s;
      l_x[mi] = x0;
      l_s[mi] = s;
      l_sc[mi] = s - K.octave_cost * log2f(K.min_pitch / (srf / x0));
    }
    __syncthreads();
    for (int mi = tid; mi < M; mi += kThreads) {
      const float sc = l_sc[mi];
      int rank = 0;
      for (int m2 = 0; m2 < M; ++m2) {
        const float o = l_sc[m2];
        rank += (o > sc || (o == sc && m2 < mi)) ? 1 : 0;
      }
      if (rank >= kCand - 1) l_lag[mi] = -l_lag[mi];                // dropped
    }
    __syncthreads();
    for (int mi = tid; mi < M; mi += kThreads) {
      if (l_lag[mi] > 0) {
        int slot = 0;
        for (int m2 = 0; m2 < mi; ++m2) slot += l_lag[m2] > 0 ? 1 : 0;
        s_sel[slot] = mi;
      }
    }
    __syncthreads();
    const int nsel = M < kCand - 1 ? M : kCand - 1;
    {
      const int grp = tid >> 4, gl = tid & 15;
      const bool live = grp < nsel;
      const int mi = live ? s_sel[grp] : 0;
      const int i0 = live ? l_lag[mi] : 2;
      double xx = live ? (double)l_x[mi] : 2.5;
      const double lo = (double)(i0 - 1), hi = (double)(i0 + 1);
#pragma unroll 1
      for (int it = 0; it < kRefineSteps; ++it) {
        const double h = it < 2 ? 0.25 : 0.125;
        const double ym = sinc_refine(fb, hw, xx - h, kDepthRefine, gl);
        const double y0 = sinc_refine(fb, hw, xx, kDepthRefine, gl);
        const double yp = sinc_refine(fb, hw, xx + h, kDepthRefine, gl);
        const double den = (2.0 * y0 - ym) - yp;
        if (den > 0.0) {
          xx = xx + 0.5 * h * (yp - ym) / den;
          xx = fmin(fmax(xx, lo), hi);
        }
      }
      double s = sinc_refine(fb, hw, xx, kDepthRefine, gl);
      if (s > 1.0) s = 1.0 / s;
      if (live && gl == 0) {
        cf[1 + grp] = (float)((double)K.sr / xx);
        cs[1 + grp] = (float)s;
      }
      if (!live && gl == 0 && grp < kCand - 1) {
        cf[1 + grp] = 0.f;
        cs[1 + grp] = 0.f;
      }
    }
    if (tid == 0) {
      cf[0] = 0.f;
      cs[0] = unvoiced;
      cand_n[g] = nsel + 1;
    }
    __syncthreads();                                                // all reads of the buffer done before the next frame
  }
}

// ---- 3. path -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void f0_path_kernel(const float* __restrict__ cand_f, const float* __restrict__ cand_s,
                                                     const int* __restrict__ cand_n, const long* __restrict__ meta,
                                                     TrackConsts K, float* __restrict__ f0,
                                                     unsigned char* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_bp[];   // 16 bytes x the longest row kept in LDS
  const int row = blockIdx.x, j = threadIdx.x;
  const long* m = meta + (long)row * T_K;
  const long T = m[T_FRAMES], foff = m[T_FOFF], bpoff = m[T_BPOFF];
  if (T <= 0) return;
  unsigned char* bp = bpoff >= 0 ? ws + bpoff : s_bp;
  const float* F = cand_f + foff * kCand;
  const float* S = cand_s + foff * kCand;
  const int* Nc = cand_n + foff;
  const bool cl = j < kCand;
  auto local_of = [&](float f, float s, bool valid, bool voiced) {
    return !valid ? -INFINITY : (voiced ? s - K.octave_cost * log2f(K.ceil_f / f) : s);
  };
  float f = cl ? F[j] : 0.f, s = cl ? S[j] : 0.f;
  int nc = Nc[0];
  bool valid = cl && j < nc, voiced = valid && f > 0.f && f < K.ceil_f;
  float lf = voiced ? log2f(f) : 0.f;
  float delta = local_of(f, s, valid, voiced);
  float nf = (cl && T > 1) ? F[kCand + j] : 0.f, nsv = (cl && T > 1) ? S[kCand + j] : 0.f;
  int nn = T > 1 ? Nc[1] : 1;
  for (long t = 1; t < T; ++t) {
    const float pf_delta = delta, pf_lf = lf;
    const int pv = voiced ? 1 : 0;
    f = nf; s = nsv; nc = nn;
    if (t + 1 < T) {                                                // in flight across this step
      if (cl) { nf = F[(t + 1) * kCand + j]; nsv = S[(t + 1) * kCand + j]; }
      nn = Nc[t + 1];
    }
    valid = cl && j < nc;
    voiced = valid && f > 0.f && f < K.ceil_f;
    lf = voiced ? log2f(f) : 0.f;
    float best = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int i = 0; i < kCand; ++i) {
      const float di = __shfl(pf_delta, i, 64);
      const float li = __shfl(pf_lf, i, 64);
      const int vi = __shfl(pv, i, 64);
      const float cost = (vi && voiced) ? K.jump_c * fabsf(li - lf) : ((vi != 0) != voiced ? K.vuv_c : 0.f);
      const float c = di - cost;
      if (c > best) { best = c; arg = i; }
    }
    delta = valid ? best + local_of(f, s, valid, voiced) : -INFINITY;
    float mx = delta;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    delta -= mx;                                                    // keeps delta O(1) on any length; path unchanged
    if (j < 16) bp[t * 16 + j] = (unsigned char)arg;
  }
  float bv = delta;
  int bi = cl ? j : 0x7fffffff;
  if (!cl) bv = -INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  if (j == 0) {
    int b = bi < 0 ? 0 : (bi > kCand - 1 ? kCand - 1 : bi);
    for (long t = T - 1; t >= 0; --t) {
      const int prev = t > 0 ? bp[t * 16 + b] : 0;
      bp[t * 16 + 15] = (unsigned char)b;
      b = prev > kCand - 1 ? kCand - 1 : prev;
    }
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  for (long t = j; t < T; t += 64) {
    const int b = bp[t * 16 + 15];
    const float fv = F[t * kCand + (b < kCand ? b : 0)];
    f0[foff + t] = (fv > 0.f && fv < K.ceil_f) ? fv : 0.f;
  }
}

size_t spill_bytes(const long* host_meta, int n_rows, long* lds_frames) {
  size_t need = 0;
  long longest = 1;
  for (int r = 0; r < n_rows; ++r) {
    const long T = host_meta[(long)r * T_K + T_FRAMES];
    if (T > kLdsFrames) need += (size_t)T * 16;
    else if (T > longest) longest = T;
  }
  *lds_frames = longest;
  return need;
}

bool meta_ok(const long* hm, int n_rows, long* total) {
  long off = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * T_K;
    if (m[T_N] < 0 || m[T_XOFF] < 0 || m[T_FRAMES] < 0 || m[T_FOFF] != off) return false;
    off += m[T_FRAMES];
  }
  *total = off;
  return true;
}

int open_batch(int n_rows, int sr, int hop, const double* config7, const long* host_meta, TrackConsts* k, long* total) {
  return open_rows(n_rows, derive(sr, hop, config7, k), host_meta, [&] { return meta_ok(host_meta, n_rows, total); },
                   total);
}

}  // namespace

extern "C" int pe_f0_track_plan_fields(void) { return T_K; }

/* Host-only layout; see include/pitchextractor_hip.h. */
extern "C" int pe_f0_track_plan(int n_rows, const long* n, const long* x_off, int sr, int hop, const double* config7,
                                long* consts8, double* dconsts2, long* meta, double* t1, long* totals2) {
  TrackConsts k;
  if (!config7 || !consts8 || !dconsts2 || !totals2 || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows > 0 && (!n || !x_off || !meta || !t1)) return PE_E_ARG;
  const int st = derive(sr, hop, config7, &k);
  if (st != PE_OK) return st;
  for (int r = 0; r < n_rows; ++r)
    if (n[r] < 0 || n[r] > (1L << 31) || x_off[r] < 0) return PE_E_ARG;
  consts8[0] = k.nw; consts8[1] = k.nper; consts8[2] = k.nfft; consts8[3] = k.maxlag; consts8[4] = k.hw;
  consts8[5] = k.hper; consts8[6] = table_floats(k); consts8[7] = kLdsFrames;
  dconsts2[0] = k.ceiling;
  dconsts2[1] = k.dt;
  long foff = 0, bpoff = 0;
  for (int r = 0; r < n_rows; ++r) {
    long* m = meta + (long)r * T_K;
    long nf;
    frame_layout(n[r], k, config7[0], &nf, &t1[r]);
    m[T_XOFF] = x_off[r]; m[T_N] = n[r]; m[T_FRAMES] = nf; m[T_FOFF] = foff;
    m[T_BPOFF] = nf > kLdsFrames ? bpoff : -1;
    if (nf > kLdsFrames) bpoff += nf * 16;
    foff += nf;
  }
  totals2[0] = foff;
  totals2[1] = bpoff;
  return PE_OK;
}

extern "C" size_t pe_row_stats_workspace_bytes(int n_rows) {
  return n_rows > 0 ? (size_t)n_rows * kChunks * (sizeof(double) + sizeof(float)) : 0;
}

extern "C" int pe_row_stats(const float* x, const long* meta, int meta_fields, int n_rows, float* stats,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || meta_fields < kRowHeader) return PE_E_ARG;
  if (n_rows == 0) return PE_OK;
  if (!x || !meta || !stats) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_row_stats_workspace_bytes(n_rows)) return PE_E_WORKSPACE;
  double* part = static_cast<double*>(workspace);
  float* pk = reinterpret_cast<float*>(part + (size_t)n_rows * kChunks);
  const dim3 pieces(kChunks, n_rows), block(kThreads);
  hipLaunchKernelGGL(f0_sum_kernel, pieces, block, 0, pe_stream(stream), x, meta, meta_fields, part);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(f0_peak_kernel, pieces, block, 0, pe_stream(stream), x, meta, meta_fields, part, pk, stats);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(f0_peak_final_kernel, dim3(pe_cdiv(n_rows, kThreads)), block, 0, pe_stream(stream), pk, n_rows,
                     stats);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_f0_track_frames(const float* x, const long* meta, const long* host_meta, const double* t1,
                                  const float* stats, const float* tables, long n_table, int n_rows, int sr, int hop,
                                  const double* config7, float* cand_f, float* cand_s, int* cand_n, void* stream) {
  TrackConsts k;
  long total = 0;
  PE_OPEN(open_batch(n_rows, sr, hop, config7, host_meta, &k, &total));
  if (!x || !meta || !t1 || !stats || !tables || !cand_f || !cand_s || !cand_n) return PE_E_ARG;
  if (n_table != table_floats(k)) return PE_E_ARG;
  return with_log2<9, 12>(k.log2c, [&](auto L) {
    hipLaunchKernelGGL(f0_frames_kernel<decltype(L)::value>, dim3(grid_of(total)), dim3(kThreads), 0, pe_stream(stream),
                       x, meta, t1, stats, tables, n_rows, total, k, cand_f, cand_s, cand_n);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

extern "C" int pe_f0_track_path(const float* cand_f, const float* cand_s, const int* cand_n, const long* meta,
                                const long* host_meta, int n_rows, int sr, int hop, const double* config7, float* f0,
                                void* workspace, size_t workspace_bytes, void* stream) {
  TrackConsts k;
  long total = 0;
  PE_OPEN(open_batch(n_rows, sr, hop, config7, host_meta, &k, &total));
  if (!cand_f || !cand_s || !cand_n || !meta || !f0) return PE_E_ARG;
  long lds_frames = 1;
  const size_t need = spill_bytes(host_meta, n_rows, &lds_frames);
  if (need > 0 && (!workspace || workspace_bytes < need)) return PE_E_WORKSPACE;
  hipLaunchKernelGGL(f0_path_kernel, dim3(n_rows), dim3(64), (size_t)lds_frames * 16, pe_stream(stream), cand_f, cand_s,
                     cand_n, meta, k, f0, static_cast<unsigned char*>(workspace));
  PE_LAUNCH_CHECK();
  return PE_OK;
}
