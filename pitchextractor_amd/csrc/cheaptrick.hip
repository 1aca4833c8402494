// WORLD CheapTrick on the GPU (Morise, Speech Communication 2015; WORLD's cheaptrick.cpp, pyworld's `cheaptrick`): the
// spectral envelope of a recording, one frame per F0 value, for a ragged batch of rows in one launch -- one workgroup
// per (row, frame), everything in LDS with the shared N-point FFT (fft_lds, dsp.h), N = fft_size in {512, 1024, 2048}.
// pe_cheaptrick_plan (host only) lays the batch out in the frame plan of world_frames.h; rows are addressed through its
// int64 table and find_row.  The DC correction and the interval mean behind the linear smoothing are world_frames.h's,
// which d4c.hip uses too; the window, the lifter and the F0 floor are this file's.
//
// Per frame, in WORLD's order: the F0-adaptive window (3 periods, sum w^2 = 1, zero DC) around the frame's sample; the
// power spectrum; the DC correction (P[k] += P interpolated at f0 - k delta for k delta <= f0); the linear smoothing of
// width 2 f0 / 3; + 2^-52; the smoothing with recovery (log, cepstrum, sinc x (1 - 2 q1 + 2 q1 cos) lifter, exp).
// Three N-point transforms per frame.  A frame's arithmetic depends on the row's samples, its F0 value and its index
// alone, and the reductions run in a fixed order: a row is bit-identical alone, at any offset, padded, anywhere in a
// batch, and whether all or some of its frames are requested.
//
// Stated deviations from WORLD: float32 per-frame arithmetic (the frame's sample origin, window length and the
// per-frame constants are derived in double); the two randn safeguards are dropped or replaced by their scale; and the
// linear smoothing is the sum over the covered bins plus the two partial edge bins, not the difference of two
// interpolated points of a cumulative sum, which in float32 drowns a quiet region in the rounding of a loud one.  In
// cell units (cell j holds P[mirror(j)] on [j, j + 1)) the interval of bin k is [k + 1/2 - h, k + 1/2 + h) with
// h = f0 N / (3 fs), so the two partial weights are the same for every bin of a frame.
#include <math.h>
#include "common.h"
#include "world_frames.h"

using namespace pe;

namespace {

constexpr int kThreads = kFrameThreads;
constexpr double kDefaultF0 = 500.0;                          // WORLD's F0 for frames at or below the floor

template <int LOG2N>
__global__ __launch_bounds__(kThreads) void cheaptrick_kernel(const float* __restrict__ x, const float* __restrict__ f0,
                                                              const long* __restrict__ meta,
                                                              const float* __restrict__ table, int n_rows,
                                                              long n_frames, double fs, double frame_period_s,
                                                              float q1, float* __restrict__ sp) {
  constexpr int N = 1 << LOG2N, H = N / 2;
  constexpr int NQ = N / kThreads, NK = H / kThreads + 1;
  __shared__ float2 s_tw[N];
  __shared__ float2 s_buf[N];
  __shared__ float s_p[H + 1];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  for (int m = tid; m < N; m += kThreads) s_tw[m] = reinterpret_cast<const float2*>(table)[m];
  __syncthreads();
  const double floor_f0 = 3.0 * fs / ((double)N - 3.0);
  for (long g = blockIdx.x; g < n_frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, FR_K, FR_FOFF, g);
    const long* m = meta + (long)row * FR_K;
    const long q = g - m[FR_FOFF], f = m[FR_FIRST] + q, n = m[FR_N];
    const float* xr = x + m[FR_XOFF];
    float* out = sp + m[FR_OOFF] + q * m[FR_OSTRIDE];
    double f0d = (double)f0[m[FR_F0OFF] + f];
    if (!(f0d > floor_f0)) f0d = kDefaultF0;
    f0d = fmin(f0d, fs * (0.5 - 1.0 / N));                      // memory safety only: F0 belongs below Nyquist
    const int half = (int)(1.5 * fs / f0d + 0.5);               // 2 half + 1 <= N - 2 above the floor
    const long origin = sample_origin((double)f * frame_period_s, fs);
    const float wstep = (float)(f0d / (1.5 * fs));
    // the window scaled to sum w^2 = 1, then the windowed wave with zero DC
    float wv[NQ], xv[NQ];
    float s_ww = 0.f;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      const int j = tid + kThreads * c;
      float w = 0.f, v = 0.f;
      if (j <= 2 * half && n > 0) {
        const int i = j - half;
        long idx = origin + i;
        idx = idx < 0 ? 0 : (idx > n - 1 ? n - 1 : idx);
        v = xr[idx];
        w = 0.5f * cospif((float)i * wstep) + 0.5f;
      }
      wv[c] = w; xv[c] = v;
      s_ww += w * w;
    }
    const float norm = sqrtf(block_sum(s_ww, s_red, tid));
    float t_w = 0.f, t_xw = 0.f;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      wv[c] = norm > 0.f ? wv[c] / norm : 0.f;
      t_w += wv[c]; t_xw += xv[c] * wv[c];
    }
    const float sum_w = block_sum(t_w, s_red, tid);
    const float sum_xw = block_sum(t_xw, s_red, tid);
    const float coef = sum_w > 0.f ? sum_xw / sum_w : 0.f;
#pragma unroll
    for (int c = 0; c < NQ; ++c) s_buf[tid + kThreads * c] = make_float2(xv[c] * wv[c] - wv[c] * coef, 0.f);
    __syncthreads();
    fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);
    for (int k = tid; k <= H; k += kThreads) {
      const float2 v = s_buf[k];
      s_p[k] = v.x * v.x + v.y * v.y;
    }
    __syncthreads();
    dc_correct<N>(s_p, f0d, fs, tid);
    // linear smoothing over [k + 1/2 - h, k + 1/2 + h) in cells, + 2^-52, log, mirrored to N points
    interval_mean<N, float, false>(s_p, [&](int k, float mean) {
      const float lq = logf(mean + 0x1p-52f);
      s_buf[k] = make_float2(lq, 0.f);
      if (k > 0 && k < H) s_buf[N - k] = make_float2(lq, 0.f);
    }, (float)(f0d * (double)N / (3.0 * fs)), tid);
    __syncthreads();
    fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);          // N x the real, even cepstrum
    {
      const float fr = (float)(f0d / fs);
      float cv[NK];
#pragma unroll
      for (int c = 0; c < NK; ++c) {
        const int i = tid + kThreads * c;
        cv[c] = 0.f;
        if (i <= H) {
          float lift = 1.f;
          if (i > 0) {
            const float a = fr * (float)i;
            lift = sinpif(a) / (kPiF * a) * ((1.f - 2.f * q1) + 2.f * q1 * cospif(2.f * a));
          }
          cv[c] = s_buf[i].x * lift / (float)N;
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NK; ++c) {
        const int i = tid + kThreads * c;
        if (i <= H) {
          s_buf[i] = make_float2(cv[c], 0.f);
          if (i > 0 && i < H) s_buf[N - i] = make_float2(cv[c], 0.f);
        }
      }
    }
    __syncthreads();
    fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);
    for (int k = tid; k <= H; k += kThreads) out[k] = expf(s_buf[k].x);
    __syncthreads();                                            // s_buf / s_p reads done before the next frame
  }
}

int config_status(double fs, double frame_period_ms, double f0_floor, int fft_size) {
  if (fft_size <= 0 || !(fs > 0.0) || !(frame_period_ms > 0.0) || !(f0_floor > 0.0) || !isfinite(fs) ||
      !isfinite(frame_period_ms) || !isfinite(f0_floor))
    return PE_E_ARG;
  if (!world_fft_size_ok(fft_size)) return PE_E_UNSUPPORTED;
  if (3.0 * fs / ((double)fft_size - 3.0) > f0_floor) return PE_E_UNSUPPORTED;   // the transform is too short for it
  return PE_OK;
}

}  // namespace

extern "C" int pe_cheaptrick_plan_fields(void) { return FR_K; }

/* Host-only batch layout; see include/pitchextractor_hip.h. */
extern "C" int pe_cheaptrick_plan(int n_rows, const long* x_off, const long* x_len, const long* f0_off,
                                  const long* f0_len, const long* first_frame, const long* n_frames,
                                  const long* out_off, const long* out_stride, double fs, double frame_period_ms,
                                  double f0_floor, int fft_size, long* meta, long* totals) {
  if (n_rows < 0 || n_rows > kMaxRows || !totals) return PE_E_ARG;
  const int st = config_status(fs, frame_period_ms, f0_floor, fft_size);
  if (st != PE_OK) return st;
  return frame_plan_fill(n_rows, x_off, x_len, f0_off, f0_len, first_frame, n_frames, out_off, out_stride, fft_size,
                         meta, totals);
}

extern "C" int pe_cheaptrick(const float* x, const float* f0, const long* meta, const long* host_meta,
                             const float* table, int n_rows, double fs, double frame_period_ms, double q1,
                             double f0_floor, int fft_size, float* sp, void* stream) {
  long frames = 0;
  PE_OPEN(open_rows(n_rows, config_status(fs, frame_period_ms, f0_floor, fft_size), host_meta,
                    [&] { return frame_plan_consistent(host_meta, n_rows, fft_size, &frames); }, &frames));
  if (!x || !f0 || !meta || !table || !sp || !isfinite(q1)) return PE_E_ARG;
  const dim3 grid(grid_for(frames, 1, 16384)), block(kThreads);
  return with_log2<9, 11>(__builtin_ctz(fft_size), [&](auto L) {
    hipLaunchKernelGGL(cheaptrick_kernel<decltype(L)::value>, grid, block, 0, pe_stream(stream), x, f0, meta, table,
                       n_rows, frames, fs, frame_period_ms / 1000.0, (float)q1, sp);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}
