// Decoding of the F0 classifier's bins back to Hz (the inverse of pe_f0_bins_ce_loss in heads_loss.hip) and the
// pitch metrics that judge the result.  Build-defined (the reference has no decoder); pinned by the float64
// restatement in tests/f0_decode_ref.py.
//   bins:     cents(b) = 20 b + 1997.3794084376191,  f(b) = 10 * 2^(cents(b) / 1200)          (CREPE's grid)
//   frames:   one wave per row: arg max with the lowest index on ties (or a bin handed in), softmax confidence of
//             that bin, and optionally the softmax-weighted average of the cents over the +-4 bins around it;
//   viterbi:  one workgroup per sequence, one thread per bin.  Transition A(i, j) = max(12 - |i - j|, 0) / rowsum_i,
//             uniform prior, ties to the lowest index.  delta lives in LDS (ping-pong), back-pointers are the signed
//             offset i - j in one byte, in LDS when T * C bytes fit and in the caller's workspace otherwise;
//   metrics:  rms cents / raw pitch accuracy / raw chroma accuracy / voicing error of a track against a reference.
// No atomics, no cross-workgroup communication.
#include "common.h"

namespace {

constexpr double kCrepeCents0 = 1997.3794084376191;      // as in heads_loss.hip
constexpr int kBand = 11;                                // transitions reach |i - j| <= 11
constexpr int kHalfWin = 4;                              // local average over b-4 .. b+4
constexpr int kMaxBins = 1024;
constexpr size_t kLdsLimit = 160 * 1024;                 // LDS of one gfx950 CU; one workgroup may take all of it

__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// (value, index) maximum over the wave, the LOWEST index among equal values; every lane gets the result
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

__device__ __forceinline__ float bin_cents(int b) { return (float)(20.0 * (double)b + kCrepeCents0); }
__device__ __forceinline__ float cents_hz(float cents) { return 10.0f * exp2f(cents / 1200.0f); }

// ------------------------------------------------------------------ frame-wise pass
// Row r = n * T + t reads logits + n * ld_n + t * ld_t once into registers (C <= 1024: 16 values per lane).
// bins_in == nullptr: the bin is the row's arg max; otherwise bins_in[r] (a Viterbi path).  Rows at
// t >= lengths[n] write zeros.
__global__ __launch_bounds__(256) void f0_decode_frames_kernel(const float* __restrict__ logits, long ld_t, long ld_n,
                                                               int C, const int* __restrict__ lengths,
                                                               const int* __restrict__ bins_in, long R, int T,
                                                               int weighted, int* __restrict__ bins_out,
                                                               float* __restrict__ f0_out,
                                                               float* __restrict__ conf_out) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * 256) >> 6;
  for (long r = wave; r < R; r += nwaves) {
    const long n = r / T;
    const int t = (int)(r - n * T);
    if (lengths != nullptr && t >= lengths[n]) {
      if (lane == 0) {
        if (bins_out) bins_out[r] = 0;
        f0_out[r] = 0.f;
        conf_out[r] = 0.f;
      }
      continue;
    }
    const float* lr = logits + n * ld_n + (long)t * ld_t;
    float v[kMaxBins / 64];
    float m = -INFINITY;
    int b = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < kMaxBins / 64; ++k) {
      const int c = k * 64 + lane;
      v[k] = (k * 64 < C && c < C) ? lr[c] : -INFINITY;
      if (v[k] > m) { m = v[k]; b = c; }
    }
    wave_argmax(m, b);
    if (bins_in != nullptr) b = bins_in[r];
    b = b < 0 ? 0 : (b > C - 1 ? C - 1 : b);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxBins / 64; ++k)
      if (k * 64 < C) s += expf(v[k] - m);                 // exp(-inf) = 0 past the end of the row
    s = wave_sum_all(s);
    const float lb = lr[b];
    float cents = bin_cents(b);
    if (weighted) {
      // average the OFFSET 20 (c - b) under the weights exp(l_c - l_b): numbers below 80 instead of around 5000
      const int c = b - kHalfWin + lane;
      float p = 0.f;
      if (lane <= 2 * kHalfWin && c >= 0 && c < C) p = expf(lr[c] - lb);
      const float num = wave_sum_all(p * (20.0f * (float)(lane - kHalfWin)));
      const float den = wave_sum_all(p);
      cents += num / den;
    }
    if (lane == 0) {
      if (bins_out) bins_out[r] = b;
      f0_out[r] = cents_hz(cents);
      conf_out[r] = expf(lb - m) / s;
    }
  }
}

// ------------------------------------------------------------------ Viterbi
// log(12 - |d|) for |d| = 0 .. 11
__device__ __constant__ float kLogTri[kBand + 1] = {
    2.48490664978800031f, 2.39789527279837054f, 2.30258509299404568f, 2.19722457733621938f,
    2.07944154167983593f, 1.94591014905531331f, 1.79175946922805500f, 1.60943791243410037f,
    1.38629436111989062f, 1.09861228866810969f, 0.69314718055994531f, 0.0f};

// sum over j in [0, C) of max(12 - |i - j|, 0): 144 in the interior, less within 11 bins of either end
__device__ __forceinline__ int tri_rowsum(int i, int C) {
  int s = 0;
  for (int d = -kBand; d <= kBand; ++d) {
    const int j = i + d;
    if (j >= 0 && j < C) s += kBand + 1 - (d < 0 ? -d : d);
  }
  return s;
}

// LDS: g[2][C + 2 * kBand] floats (g[i + kBand] = delta[i] - log rowsum_i, -inf outside [0, C)), wmax[2][16] wave
// maxima, then T * C back-pointer bytes when BP_LDS.  blockDim = C rounded up to whole waves (<= 1024).
// Frame t: thread j takes max over i in [j - 11, j + 11] of g_{t-1}[i] + log(12 - |i - j|) (first maximum = lowest
// i), adds its logit, subtracts the maximum of frame t - 1 (known to all after the previous barrier, so delta stays
// O(max logit) for any T; the path does not depend on a per-frame constant) and stores into the other buffer: one
// barrier per frame.
template <bool BP_LDS>
__global__ __launch_bounds__(1024) void f0_viterbi_kernel(const float* __restrict__ logits, long ld_t, long ld_n,
                                                          int C, const int* __restrict__ lengths, int T,
                                                          int* __restrict__ bins_out,
                                                          signed char* __restrict__ bp_global) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = blockIdx.x;
  const int j = threadIdx.x;
  const int gw = C + 2 * kBand;
  float* g = reinterpret_cast<float*>(smem);
  float* wmax = g + 2 * gw;
  signed char* bp = BP_LDS ? reinterpret_cast<signed char*>(wmax + 32) : bp_global + (long)n * T * C;
  int L = lengths != nullptr ? lengths[n] : T;
  L = L < 1 ? 1 : (L > T ? T : L);
  const float* ln = logits + (long)n * ld_n;
  const bool live = j < C;
  const int nwave = (int)blockDim.x >> 6;
  const int lane = j & 63, wv = j >> 6;

  for (int k = j; k < 2 * gw; k += blockDim.x) g[k] = -INFINITY;
  const float nlr = live ? -logf((float)tri_rowsum(j, C)) : 0.f;
  __syncthreads();
  float delta = live ? ln[j] : -INFINITY;
  float nxt = (live && L > 1) ? ln[ld_t + j] : 0.f;
  if (live) g[kBand + j] = delta + nlr;
  {
    float wm = delta;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wm = fmaxf(wm, __shfl_xor(wm, off, 64));
    if (lane == 0) wmax[wv] = wm;
  }
  __syncthreads();

  int cur = 0;
  for (int t = 1; t < L; ++t) {
    const float lt = nxt;
    if (live && t + 1 < L) nxt = ln[(long)(t + 1) * ld_t + j];       // in flight across the scan and the barrier
    float fm = wmax[cur * 16];
    for (int w = 1; w < nwave; ++w) fm = fmaxf(fm, wmax[cur * 16 + w]);
    const float* gp = g + cur * gw + j;                               // gp[d + kBand] = g[j + d]
    float best = -INFINITY;
    int arg = 0;
    if (live) {
#pragma unroll
      for (int d = -kBand; d <= kBand; ++d) {
        const float cand = gp[d + kBand] + kLogTri[d < 0 ? -d : d];
        if (cand > best) { best = cand; arg = d; }
      }
      delta = (best + lt) - fm;
      g[(cur ^ 1) * gw + kBand + j] = delta + nlr;
      bp[(long)t * C + j] = (signed char)arg;
    }
    float wm = live ? delta : -INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wm = fmaxf(wm, __shfl_xor(wm, off, 64));
    if (lane == 0) wmax[(cur ^ 1) * 16 + wv] = wm;
    cur ^= 1;
    __syncthreads();
  }

  // final state: lowest index among the maxima of delta_{L-1} (each thread still holds its own), via LDS
  if (live) g[(cur ^ 1) * gw + kBand + j] = delta;
  __syncthreads();
  if (wv == 0) {
    const float* df = g + (cur ^ 1) * gw + kBand;
    float m = -INFINITY;
    int b = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float x = df[c];
      if (x > m) { m = x; b = c; }
    }
    wave_argmax(m, b);
    if (lane == 0) {
      b = b < 0 ? 0 : (b > C - 1 ? C - 1 : b);
      int* out = bins_out + (long)n * T;
      out[L - 1] = b;
      for (int t = L - 1; t >= 1; --t) {
        b += (int)bp[(long)t * C + b];
        b = b < 0 ? 0 : (b > C - 1 ? C - 1 : b);                      // never leaves the row, whatever the logits held
        out[t - 1] = b;
      }
    }
  }
  for (int t = L + j; t < T; t += blockDim.x) bins_out[(long)n * T + t] = 0;
}

size_t viterbi_lds_fixed(int C) { return (size_t)(2 * (C + 2 * kBand) + 32) * sizeof(float); }
bool viterbi_bp_in_lds(int T, int C) { return viterbi_lds_fixed(C) + (size_t)T * C <= kLdsLimit; }

// ------------------------------------------------------------------ pitch metrics
// cents re 55 Hz (reference Utils/dynamic_pitch_tools.py:79-104), in double
__device__ __forceinline__ double cents55(double hz) { return 1200.0 * log2(hz / 55.0); }

// out[0] = rms cents over voiced reference frames (prediction clipped below at 1e-5), out[1] = raw pitch accuracy,
// out[2] = raw chroma accuracy, out[3] = voicing error share, out[4] = voiced frames, out[5] = frames
__global__ __launch_bounds__(1024) void pitch_metrics_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ ref, long n,
                                                             double threshold_cents, double* __restrict__ out) {
  __shared__ double red[5][1024];
  double sq = 0, hit = 0, chroma = 0, vuv = 0, voiced = 0;
  for (long r = threadIdx.x; r < n; r += 1024) {
    const float p = pred[r], f = ref[r];
    vuv += (p > 0.f) != (f > 0.f) ? 1.0 : 0.0;
    if (f > 0.f) {
      voiced += 1.0;
      const double d = cents55((double)fmaxf(p, 1e-5f)) - cents55((double)f);
      sq += d * d;
      if (p > 0.f) {
        hit += fabs(d) <= threshold_cents ? 1.0 : 0.0;
        double w = fmod(d + 600.0, 1200.0);
        if (w < 0.0) w += 1200.0;
        chroma += fabs(w - 600.0) <= threshold_cents ? 1.0 : 0.0;
      }
    }
  }
  red[0][threadIdx.x] = sq; red[1][threadIdx.x] = hit; red[2][threadIdx.x] = chroma;
  red[3][threadIdx.x] = vuv; red[4][threadIdx.x] = voiced;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < 5; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nv = red[4][0];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[0] = nv > 0 ? sqrt(red[0][0] / nv) : nan;
    out[1] = nv > 0 ? red[1][0] / nv : nan;
    out[2] = nv > 0 ? red[2][0] / nv : nan;
    out[3] = red[3][0] / (double)n;
    out[4] = nv;
    out[5] = (double)n;
  }
}

bool decode_shape_ok(const float* logits, long ld_t, long ld_n, int C, int N, int T) {
  return logits && N > 0 && T > 0 && C >= 2 && ld_t >= C && ld_n >= (long)(T - 1) * ld_t + C;
}

}  // namespace

extern "C" int pe_f0_decode_frames(const float* logits, long ld_t, long ld_n, int C, const int* lengths,
                                   const int* bins_in, int N, int T, int method, int* bins_out, float* f0_out,
                                   float* conf_out, void* stream) {
  if (!decode_shape_ok(logits, ld_t, ld_n, C, N, T) || !f0_out || !conf_out || (!bins_in && !bins_out))
    return PE_E_ARG;
  if (method != PE_F0_ARGMAX && method != PE_F0_WEIGHTED) return PE_E_ARG;
  if (C > kMaxBins) return PE_E_UNSUPPORTED;
  const long R = (long)N * T;
  long grid = (R + 3) / 4;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(f0_decode_frames_kernel, dim3((int)grid), dim3(256), 0, pe_stream(stream), logits, ld_t, ld_n, C,
                     lengths, bins_in, R, T, method == PE_F0_WEIGHTED ? 1 : 0, bins_out, f0_out, conf_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" size_t pe_f0_viterbi_workspace_bytes(int N, int T, int C) {
  if (N <= 0 || T <= 0 || C < 2 || C > kMaxBins || viterbi_bp_in_lds(T, C)) return 0;
  return (size_t)N * T * C;
}

extern "C" int pe_f0_viterbi(const float* logits, long ld_t, long ld_n, int C, const int* lengths, int N, int T,
                             int* bins_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!decode_shape_ok(logits, ld_t, ld_n, C, N, T) || !bins_out) return PE_E_ARG;
  if (C > kMaxBins) return PE_E_UNSUPPORTED;
  const size_t need = pe_f0_viterbi_workspace_bytes(N, T, C);
  if (need > 0 && (!workspace || workspace_bytes < need)) return PE_E_WORKSPACE;
  const int threads = ((C + 63) / 64) * 64;
  if (need == 0) {
    const size_t lds = viterbi_lds_fixed(C) + (size_t)T * C;
    static size_t attr = 0;                                  // the largest LDS size the kernel has been allowed
    if (lds > attr) {
      PE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&f0_viterbi_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
      attr = kLdsLimit;
    }
    hipLaunchKernelGGL(f0_viterbi_kernel<true>, dim3(N), dim3(threads), lds, pe_stream(stream), logits, ld_t, ld_n, C,
                       lengths, T, bins_out, static_cast<signed char*>(nullptr));
  } else {
    hipLaunchKernelGGL(f0_viterbi_kernel<false>, dim3(N), dim3(threads), viterbi_lds_fixed(C), pe_stream(stream),
                       logits, ld_t, ld_n, C, lengths, T, bins_out, static_cast<signed char*>(workspace));
  }
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_pitch_metrics(const float* f0_pred, const float* f0_ref, long n, double threshold_cents,
                                double* out6, void* stream) {
  if (!f0_pred || !f0_ref || !out6 || n <= 0 || !(threshold_cents >= 0.0)) return PE_E_ARG;
  hipLaunchKernelGGL(pitch_metrics_kernel, dim3(1), dim3(1024), 0, pe_stream(stream), f0_pred, f0_ref, n,
                     threshold_cents, out6);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
