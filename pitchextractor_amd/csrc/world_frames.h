// What the two WORLD frame analyses (cheaptrick.hip, d4c.hip) share on top of dsp.h.  Host: the transform sizes the
// WORLD entry points take (world_synth.hip's too), and the frame plan: one row table, one fill, one consistency walk,
// so a `meta` from pe_cheaptrick_plan or pe_d4c_plan is one layout that pe_cheaptrick, pe_d4c_bands and pe_d4c_expand
// all accept.  Device, for a workgroup of kFrameThreads threads that holds a frame's N / 2 + 1 bins in LDS: the frame's
// sample origin, CheapTrick's DC correction, and its linear smoothing as the mean over an interval of cells.
#pragma once
#include <math.h>
#include "dsp.h"

namespace pe {

constexpr int kFrameThreads = 256;

inline bool world_fft_size_ok(int n) { return n == 512 || n == 1024 || n == 2048; }

// per-row frame plan fields (int64): the row's offset in x and its length, the offset of its F0 curve, the first frame
// and the number of frames analysed, their prefix over the batch, and where frame q goes: FR_OOFF + q * FR_OSTRIDE
enum { FR_XOFF, FR_N, FR_F0OFF, FR_FIRST, FR_FRAMES, FR_FOFF, FR_OOFF, FR_OSTRIDE, FR_K };
static_assert(FR_XOFF == kRowOffset && FR_N == kRowLength, "a row plan opens with offset and length");

// The body of a pe_*_plan after its own range and config checks: null arrays or a row out of range is PE_E_ARG; else
// meta is filled and *frames is the batch's frame total.  fields: int64 per row of meta, for a plan that appends fields
// of its own to these (world_warp.hip).
inline int frame_plan_fill(int n_rows, const long* x_off, const long* x_len, const long* f0_off, const long* f0_len,
                           const long* first_frame, const long* n_frames, const long* out_off,
                           const long* out_stride, int fft_size, long* meta, long* frames, int fields = FR_K) {
  if (n_rows > 0 && (!x_off || !x_len || !f0_off || !f0_len || !first_frame || !n_frames || !out_off || !out_stride ||
                     !meta))
    return PE_E_ARG;
  const long bins = fft_size / 2 + 1;
  long tot = 0;
  for (int r = 0; r < n_rows; ++r) {
    if (x_off[r] < 0 || x_len[r] < 0 || x_len[r] > (1L << 31) || f0_off[r] < 0 || f0_len[r] < 0 ||
        f0_len[r] > (1L << 31) || first_frame[r] < 0 || n_frames[r] < 0 || first_frame[r] + n_frames[r] > f0_len[r] ||
        out_off[r] < 0 || out_stride[r] < bins || (n_frames[r] > 0 && x_len[r] < 1))
      return PE_E_ARG;
    long* m = meta + (long)r * fields;
    m[FR_XOFF] = x_off[r]; m[FR_N] = x_len[r]; m[FR_F0OFF] = f0_off[r]; m[FR_FIRST] = first_frame[r];
    m[FR_FRAMES] = n_frames[r]; m[FR_FOFF] = tot; m[FR_OOFF] = out_off[r]; m[FR_OSTRIDE] = out_stride[r];
    tot += n_frames[r];
  }
  *frames = tot;
  return PE_OK;
}

// the plan's own walk over its host copy: what the kernels' addressing relies on; fills {frames}
inline bool frame_plan_consistent(const long* hm, int n_rows, int fft_size, long* frames, int fields = FR_K) {
  long tot = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * fields;
    if (m[FR_XOFF] < 0 || m[FR_N] < 0 || m[FR_F0OFF] < 0 || m[FR_FIRST] < 0 || m[FR_FRAMES] < 0 ||
        m[FR_FOFF] != tot || m[FR_OOFF] < 0 || m[FR_OSTRIDE] < fft_size / 2 + 1 || (m[FR_FRAMES] > 0 && m[FR_N] < 1))
      return false;
    tot += m[FR_FRAMES];
  }
  *frames = tot;
  return true;
}

__device__ __forceinline__ long matlab_round(double v) { return v > 0.0 ? (long)(v + 0.5) : (long)(v - 0.5); }

// WORLD's sample of the time t seconds
__device__ __forceinline__ long sample_origin(double t, double fs) { return matlab_round(t * fs + 0.001); }

// CheapTrick's DC correction in place: p[k] += p interpolated at r - k for k <= K (r = f0 N / fs in bins), the replica
// from the uncorrected values.  The workgroup has met when it returns.
template <int N>
__device__ __forceinline__ void dc_correct(float* s_p, double f0d, double fs, int tid) {
  constexpr int H = N / 2, NK = H / kFrameThreads + 1;
  int K = (int)(f0d / (fs / (double)N));
  K = K < H - 1 ? K : H - 1;
  const float r = (float)(f0d * (double)N / fs);
  float rep[NK];
#pragma unroll
  for (int c = 0; c < NK; ++c) {
    const int k = tid + kFrameThreads * c;
    rep[c] = 0.f;
    if (k <= K) {
      const float pos = r - (float)k;
      int base = (int)floorf(pos);
      const float frac = pos - (float)base;
      base = base < 0 ? 0 : (base > H - 1 ? H - 1 : base);
      const float p0 = s_p[base], p1 = s_p[base + 1];
      rep[c] = p0 + (p1 - p0) * frac;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NK; ++c) {
    const int k = tid + kFrameThreads * c;
    if (k <= K) s_p[k] += rep[c];
  }
  __syncthreads();
}

// CheapTrick's linear smoothing at half width h bins: put(k, mean of src over [k + 1/2 - h, k + 1/2 + h) in cells) for
// k <= N / 2, where cell j holds src[mirror(j)] on [j, j + 1): the whole cells plus the two partial ones at the ends,
// whose weights are the same for every bin.  put does not write src; the caller meets after it.  The sum is accumulated
// in Acc and rounded once.  SEED: the first partial cell opens the running sum (d4c.hip); without it the whole cells
// are summed on their own and added to it (cheaptrick.hip).  Those are two roundings of the same sum, and each analysis
// keeps the one its recorded bits were made with (tests/test_world_frames_parity_gpu.py).
template <int N, class Acc, bool SEED, class Put>
__device__ __forceinline__ void interval_mean(const float* src, Put&& put, float h, int tid) {
  constexpr int H = N / 2;
  const int hi = (int)floorf(h);
  const float hf = h - (float)hi;
  const bool lo_down = hf > 0.5f, up = hf >= 0.5f;
  const int ka_off = -hi - (lo_down ? 1 : 0), kb_off = hi + (up ? 1 : 0);
  const float wa = 1.f - (lo_down ? 1.5f - hf : 0.5f - hf);
  const float wb = up ? hf - 0.5f : 0.5f + hf;
  auto cell = [&](int j) {
    j = j < 0 ? -j : j;
    j = j > H ? N - j : j;
    return (Acc)src[j < 0 ? 0 : j];
  };
  for (int k = tid; k <= H; k += kFrameThreads) {
    const int ka = k + ka_off, kb = k + kb_off;
    Acc s;
    if (ka == kb) {
      s = (Acc)2 * (Acc)h * cell(ka);
    } else {
      s = (Acc)wa * cell(ka);
      if constexpr (SEED) {
        for (int j = ka + 1; j < kb; ++j) s += cell(j);
      } else {
        Acc mid = 0;
        for (int j = ka + 1; j < kb; ++j) mid += cell(j);
        if (kb - ka > 1) s += mid;
      }
      s += (Acc)wb * cell(kb);
    }
    put(k, (float)(s / ((Acc)2 * (Acc)h)));
  }
}

}  // namespace pe
