// WORLD D4C on the GPU (Morise, Speech Communication 84, 2016; WORLD's d4c.cpp, pyworld's `d4c`): the band aperiodicity
// of a recording, one frame per F0 value, for a ragged batch of rows.  pe_d4c_plan (host only) lays the batch out in
// the frame plan of world_frames.h, as pe_cheaptrick_plan does; pe_d4c_bands is one launch with one workgroup per
// (row, frame), everything in LDS with the shared FFT (fft_lds, dsp.h) at N_d = 2^(1 + floor(log2(4 fs / 47 + 1))) in
// {2048, 4096}; pe_d4c_expand is one launch that interpolates a frame's band values to the fft_size / 2 + 1 bins the
// synthesizer reads.
//
// Per frame, in WORLD's order.  LoveTrain: the Blackman window of 3 periods at max(F0, 40) around the frame's sample,
// zero-padded to N_l = 2^(1 + floor(log2(3 fs / 40 + 1))) (N_d or N_d / 2), |X|^2, a0 = sum over [100 Hz, 4000 Hz] /
// sum over [100 Hz, 7900 Hz] in bins rounded up.  F0 <= 0 (or not a number) or a0 <= threshold: the unvoiced verdict.
// Otherwise, with f0 = max(47, F0): the smoothed power (Hanning window of 4 periods, DC correction, linear smoothing of
// width f0); the static centroid (Blackman windows of 4 periods at t -+ 1 / (4 f0), each scaled to unit energy, Re X Re
// Y + Im X Im Y with Y the transform of the wave times its sample number, the two added and DC-corrected); the static
// group delay (centroid / power, smoothed over f0 / 2, minus its own smoothing over f0); per 3 kHz band the Nuttall-
// windowed group delay's power spectrum, sorted, and coarse = 10 log10 of the share of all but the largest
// round(8 N_d / L) + 1 values; coarse <- min(0, coarse + (F0 - 100) / 50).
//
// Real transforms ride two to one on the complex one where the pair is at hand: a centroid's wave and its ramped copy
// (the ramp scaled by a power of two so that both halves have the same magnitude), and two bands.  The sort is bitonic
// in LDS over N_d values (N_d / 2 + 1 powers, the rest +inf), two bands side by side in the transform's buffer; the
// sums that stand for WORLD's cumulative sums run over a thread's contiguous values and then the workgroup's fixed
// tree.  No atomics, no traffic between workgroups: a row is bit-identical alone, at any offset, padded, anywhere in a
// batch, and whether all or some of its frames are requested.
//
// Stated deviations from WORLD: float32 per-frame arithmetic (sample origins, window lengths and per-frame constants
// are formed in double); the randn * 1e-12 of the window is dropped, and a frame whose LoveTrain denominator is 0 has
// a0 = 0, one whose smoothed power is not positive in every bin takes the unvoiced verdict; the linear smoothing is
// the interval mean CheapTrick uses (world_frames.h, where the DC correction is too) at a general width, which serves
// the signed centroid unchanged, its sum accumulated in double.  A band whose group delay is all zero reads 0 dB, and
// coarse is floored at -200 dB so that no -inf reaches the interpolation.
#include <math.h>
#include "common.h"
#include "world_frames.h"

using namespace pe;

namespace {

constexpr int kThreads = kFrameThreads;
constexpr double kFloorF0 = 47.0, kLowestF0 = 40.0;           // band analysis / LoveTrain
constexpr double kInterval = 3000.0, kUpperLimit = 15000.0;
constexpr float kSafe = 1e-12f;
constexpr int kMaxBands = 5, kMaxN = 4096;

struct Derived {
  int n_d, n_l, bands, L;
};

int pow2_above(double v) {                                     // 2^(1 + floor(log2(v))), v >= 1
  int n = 2;
  while ((double)n <= v) n *= 2;
  return n;
}

int config_status(double fs, double frame_period_ms, int fft_size, Derived* d) {
  if (fft_size <= 0 || !(fs > 0.0) || !(frame_period_ms > 0.0) || !isfinite(fs) || !isfinite(frame_period_ms))
    return PE_E_ARG;
  if (!world_fft_size_ok(fft_size)) return PE_E_UNSUPPORTED;
  if (fs / 2.0 <= 7900.0 || fs > 1e6) return PE_E_UNSUPPORTED;    // the LoveTrain band would leave the spectrum
  Derived v;
  v.n_d = pow2_above(4.0 * fs / kFloorF0 + 1.0);
  v.n_l = pow2_above(3.0 * fs / kLowestF0 + 1.0);
  v.bands = (int)(fmin(kUpperLimit, fs / 2.0 - kInterval) / kInterval);
  v.L = 2 * (int)(kInterval * v.n_d / fs) + 1;
  if (v.n_d > kMaxN || v.n_l > kMaxN || v.bands > kMaxBands || v.bands < 1) return PE_E_UNSUPPORTED;
  if (d) *d = v;
  return PE_OK;
}

// WORLD's GetWindowedWaveform without its randn: samples j = tid + 256 c < len of the window of `ratio` periods of f0
// around `pos` seconds (Blackman, or Hanning), times the wave, minus the window times sum(x w) / sum(w).
template <int NQ>
__device__ __forceinline__ void windowed_wave(const float* __restrict__ xr, long n, double fs, double f0d, double pos,
                                              double ratio, bool blackman, int max_len, float* s_red, int tid,
                                              float (&wave)[NQ], int& len) {
  const int half = (int)matlab_round(ratio * fs / f0d / 2.0);
  len = 2 * half + 1 < max_len ? 2 * half + 1 : max_len;
  const long origin = sample_origin(pos, fs);
  const float wstep = (float)(2.0 * f0d / (ratio * fs));
  float wv[NQ];
  float t_w = 0.f, t_xw = 0.f;
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const int j = tid + kThreads * c;
    float w = 0.f, v = 0.f;
    if (j < len) {
      const int i = j - half;
      long idx = origin + i;
      idx = idx < 0 ? 0 : (idx > n - 1 ? n - 1 : idx);
      const float a = (float)i * wstep;
      w = blackman ? 0.08f * cospif(2.f * a) + 0.5f * cospif(a) + 0.42f : 0.5f * cospif(a) + 0.5f;
      v = xr[idx] * w;
    }
    wv[c] = w; wave[c] = v;
    t_w += w; t_xw += v;
  }
  const float sum_w = block_sum(t_w, s_red, tid);
  const float sum_xw = block_sum(t_xw, s_red, tid);
  const float coef = sum_w > 0.f ? sum_xw / sum_w : 0.f;
#pragma unroll
  for (int c = 0; c < NQ; ++c) wave[c] -= wv[c] * coef;
}

// tw <- the first 3 C / 4 of the C-th roots of unity (all that fft_lds reads)
__device__ __forceinline__ void load_roots(float2* s_tw, const float* table, int C, int tid) {
  for (int m = tid; m < 3 * C / 4; m += kThreads) s_tw[m] = reinterpret_cast<const float2*>(table)[m];
}

// LoveTrain's a0 of a frame; LOG2L: log2 of N_l, whose roots s_tw holds
template <int LOG2L, int NQ>
__device__ __forceinline__ float love_train(const float* __restrict__ xr, long n, double fs, double f0d, double pos,
                                            float2* s_buf, const float2* s_tw, float* s_red, int tid) {
  constexpr int NL = 1 << LOG2L;
  float wave[NQ];
  int len;
  windowed_wave<NQ>(xr, n, fs, f0d, pos, 3.0, true, NL, s_red, tid, wave, len);
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const int j = tid + kThreads * c;
    if (j < NL) s_buf[j] = make_float2(wave[c], 0.f);
  }
  __syncthreads();
  fft_lds<LOG2L, false, kThreads>(s_buf, s_tw, tid);
  const int b0 = (int)ceil(100.0 * NL / fs), b1 = (int)ceil(4000.0 * NL / fs), b2 = (int)ceil(7900.0 * NL / fs);
  float num = 0.f, den = 0.f;
  for (int k = b0 + tid; k <= b2 && k <= NL / 2; k += kThreads) {
    const float2 v = s_buf[k];
    const float p = v.x * v.x + v.y * v.y;
    den += p;
    if (k <= b1) num += p;
  }
  num = block_sum(num, s_red, tid);
  den = block_sum(den, s_red, tid);
  return den > 0.f ? num / den : 0.f;
}

// The linear smoothing at half width h bins: dst <- interval_mean of src (dst is not src; the caller meets after it),
// accumulated in double and rounded once: at F0 = 1000 Hz the sum has 85 terms, the group delay's second smoothing is
// subtracted from the first, and a float32 running sum costs the band values four times what every other stage together
// does (tools/d4c_noise_study.py).
template <int N>
__device__ __forceinline__ void smooth(const float* src, float* dst, float h, int tid) {
  interval_mean<N, double, true>(src, [&](int k, float mean) { dst[k] = mean; }, h, tid);
}

template <int LOG2N>
__global__ __launch_bounds__(kThreads) void d4c_bands_kernel(const float* __restrict__ x, const float* __restrict__ f0,
                                                             const long* __restrict__ meta,
                                                             const float* __restrict__ table, int n_rows,
                                                             long n_frames, double fs, double frame_period_s,
                                                             float threshold, int n_l, int bands, int L,
                                                             float* __restrict__ out) {
  constexpr int N = 1 << LOG2N, H = N / 2;
  constexpr int NQ = N / kThreads, NK = H / kThreads + 1;
  __shared__ float2 s_tw[3 * N / 4];
  __shared__ float2 s_buf[N];
  __shared__ float s_a[H + 1];
  __shared__ float s_b[H + 1];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  const float* table_l = table + 2 * N;                          // the N_l-th roots follow the N_d-th
  const bool same = n_l == N;
  if (same) load_roots(s_tw, table, N, tid);
  __syncthreads();
  for (long g = blockIdx.x; g < n_frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, FR_K, FR_FOFF, g);
    const long* m = meta + (long)row * FR_K;
    const long f = m[FR_FIRST] + (g - m[FR_FOFF]), n = m[FR_N];
    const float* xr = x + m[FR_XOFF];
    float* o = out + g * (1 + bands);
    const float f0f = f0[m[FR_F0OFF] + f];
    const double t = (double)f * frame_period_s;
    const bool f0_ok = f0f > 0.f;
    // ---- LoveTrain
    float a0 = 0.f;
    if (f0_ok) {
      const double fl = fmin(fmax((double)f0f, kLowestF0), fs * (0.5 - 1.0 / n_l));
      if (same) {
        a0 = love_train<LOG2N, NQ>(xr, n, fs, fl, t, s_buf, s_tw, s_red, tid);
      } else {
        __syncthreads();
        load_roots(s_tw, table_l, N / 2, tid);
        __syncthreads();
        a0 = love_train<LOG2N - 1, NQ>(xr, n, fs, fl, t, s_buf, s_tw, s_red, tid);
      }
    }
    bool voiced = f0_ok && !(a0 <= threshold);
    if (voiced) {
      if (!same) {
        __syncthreads();
        load_roots(s_tw, table, N, tid);
      }
      __syncthreads();
      const double fd = fmin(fmax((double)f0f, kFloorF0), fs * (0.5 - 1.0 / N));   // the upper bound: memory safety
      float wave[NQ];
      int len;
      // ---- the smoothed power -> s_b
      windowed_wave<NQ>(xr, n, fs, fd, t, 4.0, false, N, s_red, tid, wave, len);
#pragma unroll
      for (int c = 0; c < NQ; ++c) s_buf[tid + kThreads * c] = make_float2(wave[c], 0.f);
      __syncthreads();
      fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);
      for (int k = tid; k <= H; k += kThreads) {
        const float2 v = s_buf[k];
        s_a[k] = v.x * v.x + v.y * v.y;
      }
      __syncthreads();
      dc_correct<N>(s_a, fd, fs, tid);
      smooth<N>(s_a, s_b, (float)(fd * (double)N / (2.0 * fs)), tid);
      __syncthreads();
      float bad = 0.f;
      for (int k = tid; k <= H; k += kThreads) bad = fmaxf(bad, s_b[k] > 0.f ? 0.f : 1.f);
      voiced = block_max(bad, s_red, tid) == 0.f;
    }
    if (!voiced) {                                               // uniform: every thread holds the same a0 and flags
      if (tid <= bands) o[tid] = tid == 0 ? a0 : __builtin_nanf("");
      continue;
    }
    const double fd = fmin(fmax((double)f0f, kFloorF0), fs * (0.5 - 1.0 / N));
    // ---- the static centroid -> s_a: the wave and its ramped copy as one complex signal, at t -+ 1 / (4 f0)
    for (int side = 0; side < 2; ++side) {
      float wave[NQ];
      int len;
      windowed_wave<NQ>(xr, n, fs, fd, t + (side ? 0.25 : -0.25) / fd, 4.0, true, N, s_red, tid, wave, len);
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < NQ; ++c) ss += wave[c] * wave[c];
      ss = block_sum(ss, s_red, tid);
      const float scale = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
      const int p2 = 32 - __builtin_clz(len);                      // the ramp 1 .. len times 2^-p2 stays below 1
      const float ramp = ldexpf(1.f, -p2);
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        const int j = tid + kThreads * c;
        const float w = wave[c] * scale;
        s_buf[j] = make_float2(w, w * ((float)(j + 1) * ramp));
      }
      __syncthreads();
      fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);
      const float back = ldexpf(1.f, p2);
      for (int k = tid; k <= H; k += kThreads) {
        float2 X, Y;
        real_fft_split(s_buf[k], conj2(s_buf[(N - k) & (N - 1)]), X, Y);
        const float cen = (X.x * Y.x + X.y * Y.y) * back;
        s_a[k] = side ? s_a[k] + cen : cen;
      }
      __syncthreads();
    }
    dc_correct<N>(s_a, fd, fs, tid);
    // ---- the static group delay: g = centroid / power; g <- smooth(g, f0 / 2); g <- g - smooth(g, f0) -> s_a
    for (int k = tid; k <= H; k += kThreads) s_a[k] = s_a[k] / s_b[k];
    __syncthreads();
    smooth<N>(s_a, s_b, (float)(fd * (double)N / (4.0 * fs)), tid);
    __syncthreads();
    smooth<N>(s_b, s_a, (float)(fd * (double)N / (2.0 * fs)), tid);
    __syncthreads();
    for (int k = tid; k <= H; k += kThreads) s_a[k] = s_b[k] - s_a[k];
    __syncthreads();
    // ---- the bands, two per transform
    const int hl = L / 2;
    int bw = (int)(8.0 * N / L + 0.5);
    bw = bw < H - 1 ? bw : H - 1;
    float* sort = reinterpret_cast<float*>(s_buf);                 // two arrays of N floats
    for (int b = 0; b < bands; b += 2) {
      const bool two = b + 1 < bands;
      const int ca = (int)(kInterval * (b + 1) * N / fs) - hl, cb = (int)(kInterval * (b + 2) * N / fs) - hl;
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        const int j = tid + kThreads * c;
        float2 v = make_float2(0.f, 0.f);
        if (j < L) {
          const float u = (float)j / (float)(L - 1);
          const float w = 0.355768f - 0.487396f * cospif(2.f * u) + 0.144232f * cospif(4.f * u) -
                          0.012604f * cospif(6.f * u);
          v.x = s_a[ca + j] * w;
          if (two) v.y = s_a[cb + j] * w;
        }
        s_buf[j] = v;
      }
      __syncthreads();
      fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);
      float pa[NK], pb[NK];
#pragma unroll
      for (int c = 0; c < NK; ++c) {
        const int k = tid + kThreads * c;
        pa[c] = pb[c] = 0.f;
        if (k <= H) {
          float2 A, B;
          real_fft_split(s_buf[k], conj2(s_buf[(N - k) & (N - 1)]), A, B);
          pa[c] = A.x * A.x + A.y * A.y;
          pb[c] = B.x * B.x + B.y * B.y;
        }
      }
      __syncthreads();
      const int arrays = two ? 2 : 1;
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        const int k = tid + kThreads * c;
        float va = INFINITY, vb = INFINITY;
        if (k <= H) { va = pa[c < NK ? c : 0]; vb = pb[c < NK ? c : 0]; }      // k <= H only where c < NK
        sort[k] = va;
        if (two) sort[N + k] = vb;
      }
      __syncthreads();
      // bitonic, ascending in each array of N (the last merge runs upwards in both).  A step's pairs are disjoint:
      // a thread reads all of its pairs before it writes any, so the reads are in flight together
      for (int kk = 2; kk <= N; kk <<= 1) {
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
          float u[NQ], v[NQ];
#pragma unroll
          for (int c = 0; c < NQ; ++c) {
            const int q = tid + kThreads * c;
            if (q < arrays * H) {
              const int i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1));
              u[c] = sort[i]; v[c] = sort[i | jj];
            }
          }
#pragma unroll
          for (int c = 0; c < NQ; ++c) {
            const int q = tid + kThreads * c;
            if (q < arrays * H) {
              const int i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1));
              const bool asc = kk == N || (i & kk) == 0;
              if ((u[c] > v[c]) == asc) { sort[i] = v[c]; sort[i | jj] = u[c]; }
            }
          }
          __syncthreads();
        }
      }
      // S[H - bw - 1] and S[H] of the ascending cumulative sum: a thread's NQ contiguous values, then the tree
      for (int a = 0; a < arrays; ++a) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          const int k = tid * NQ + c;
          const float v = k <= H ? sort[a * N + k] : 0.f;
          s2 += v;
          if (k <= H - bw - 1) s1 += v;
        }
        s1 = block_sum(s1, s_red, tid);
        s2 = block_sum(s2, s_red, tid);
        float coarse = s2 > 0.f ? fmaxf(10.f * log10f(s1 / s2), -200.f) : 0.f;
        coarse = fminf(0.f, coarse + (f0f - 100.f) / 50.f);
        if (tid == 0) o[1 + b + a] = coarse;
      }
      __syncthreads();
    }
    if (tid == 0) o[0] = a0;
  }
}

// knots (0, -60), (3000 (i + 1), coarse[i]) ..., (fs / 2, -safe) in dB, interpolated at k fs / fft_size, 10^(dB / 20)
__global__ __launch_bounds__(kThreads) void d4c_expand_kernel(const float* __restrict__ band, const long* __restrict__ meta,
                                                              int n_rows, long n_frames, double fs, int fft_size,
                                                              int bands, float* __restrict__ ap) {
  const int bins = fft_size / 2 + 1;
  for (long g = blockIdx.x; g < n_frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, FR_K, FR_FOFF, g);
    const long* m = meta + (long)row * FR_K;
    float* out = ap + m[FR_OOFF] + (g - m[FR_FOFF]) * m[FR_OSTRIDE];
    const float* c = band + g * (1 + bands) + 1;
    const bool unvoiced = !(c[0] == c[0]);
    for (int k = threadIdx.x; k < bins; k += kThreads) {
      float v = 1.f - kSafe;
      if (!unvoiced) {
        const float fr = (float)((double)k * fs / fft_size);
        int seg = (int)(fr / (float)kInterval);
        seg = seg > bands ? bands : seg;
        const float x_lo = (float)kInterval * seg, x_hi = seg == bands ? (float)(fs / 2.0) : (float)kInterval * (seg + 1);
        const float y_lo = seg == 0 ? -60.f : c[seg - 1], y_hi = seg == bands ? -kSafe : c[seg];
        const float db = fminf((y_hi - y_lo) / (x_hi - x_lo) * (fr - x_lo) + y_lo, 0.f);   // no knot lies above 0
        v = exp10f(db / 20.f);
      }
      out[k] = v;
    }
  }
}

}  // namespace

extern "C" int pe_d4c_plan_fields(void) { return FR_K; }

/* Host-only batch layout; see include/pitchextractor_hip.h. */
extern "C" int pe_d4c_plan(int n_rows, const long* x_off, const long* x_len, const long* f0_off, const long* f0_len,
                           const long* first_frame, const long* n_frames, const long* out_off, const long* out_stride,
                           double fs, double frame_period_ms, int fft_size, long* meta, long* totals) {
  if (n_rows < 0 || n_rows > kMaxRows || !totals) return PE_E_ARG;
  Derived d;
  int st = config_status(fs, frame_period_ms, fft_size, &d);
  if (st != PE_OK) return st;
  if ((st = frame_plan_fill(n_rows, x_off, x_len, f0_off, f0_len, first_frame, n_frames, out_off, out_stride, fft_size,
                            meta, totals)) != PE_OK)
    return st;
  totals[1] = d.n_d; totals[2] = d.n_l; totals[3] = d.bands; totals[4] = d.L;
  return PE_OK;
}

extern "C" int pe_d4c_bands(const float* x, const float* f0, const long* meta, const long* host_meta,
                            const float* table, int n_rows, double fs, double frame_period_ms, double threshold,
                            int fft_size, float* band, void* stream) {
  long frames = 0;
  Derived d = {};
  if (!isfinite(threshold)) return PE_E_ARG;
  PE_OPEN(open_rows(n_rows, config_status(fs, frame_period_ms, fft_size, &d), host_meta,
                    [&] { return frame_plan_consistent(host_meta, n_rows, fft_size, &frames); }, &frames));
  if (!x || !f0 || !meta || !table || !band) return PE_E_ARG;
  const dim3 grid(grid_for(frames, 1, 16384)), block(kThreads);
  return with_log2<11, 12>(__builtin_ctz(d.n_d), [&](auto L2) {
    hipLaunchKernelGGL(d4c_bands_kernel<decltype(L2)::value>, grid, block, 0, pe_stream(stream), x, f0, meta, table,
                       n_rows, frames, fs, frame_period_ms / 1000.0, (float)threshold, d.n_l, d.bands, d.L, band);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

extern "C" int pe_d4c_expand(const float* band, const long* meta, const long* host_meta, int n_rows, double fs,
                             int fft_size, float* ap, void* stream) {
  long frames = 0;
  Derived d = {};
  PE_OPEN(open_rows(n_rows, config_status(fs, 1.0, fft_size, &d), host_meta,
                    [&] { return frame_plan_consistent(host_meta, n_rows, fft_size, &frames); }, &frames));
  if (!band || !meta || !ap) return PE_E_ARG;
  hipLaunchKernelGGL(d4c_expand_kernel, dim3(grid_for(frames, 1, 65536)), dim3(kThreads), 0, pe_stream(stream), band,
                     meta, n_rows, frames, fs, fft_size, d.bands, ap);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
