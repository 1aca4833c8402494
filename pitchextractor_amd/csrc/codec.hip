// Codec stress conditions of the reference's Utils/codec_and_bandwidth_torture.ipynb on ragged batches: a build-defined
// MDCT transform codec ("ptc": what opus, mp3 and aac have in common, not their bitstreams) and G.711 mu-law.  The
// specification is DESIGN.md section 28; tests/codec_ref.py restates it in numpy.
//
// pe_codec_plan (host only) lays the rows out: offset and length (the shared row header), the row's offset in the
// output, its frames F = ceil(n / M) + 1 (none for an empty row) and their prefix.  Frame f of a row reads the 2M
// samples from (f - 1) M on, zero outside the row.  One workgroup of 256 threads per (row, frame), everything in LDS:
//   mdct:      window, fold the 2M samples to M, DCT-IV through the M / 2-point complex fft_lds of dsp.h with one
//              twiddle exp(-i pi (8 n + 1) / 8M) ahead of it and behind it.
//   quantize:  the band maxima (integer atomicMax on the bit pattern of |X|: exact, order-free), the step index per
//              band, the eight-step bisection over the global gain g (cost is non-increasing in g) and the pass that
//              writes q and the dequantised values.  Integer sums only, so the order of the atomics is free.
//   imdct:     DCT-IV again (it is its own inverse up to 2 / M), unfold to 2M, window: the windowed frame goes to a
//              scratch of (frames, 2M); a second launch gathers output block b of a row as the second half of frame b
//              plus the first half of frame b + 1.  No atomics on the output; every sample is written once.
//   apply:     the three chained in one launch on the coefficients in LDS (the same device functions, so the result
//              is that of the three stage calls bit for bit), then the same gather.
//   mulaw:     elementwise, integers.
// The whole file is compiled without floating-point contraction: a stage gives the same bits in whichever kernel it is
// inlined.  Nothing a row computes depends on where the row lies: it is the same alone, packed or padded.
#pragma clang fp contract(off)
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBands = 48;                     // 29 / 35 / 41 bands at M = 256 / 512 / 1024
constexpr int kSteps = 448, kStepBias = 160;      // the step tables T and R; i = g + floor(2 s / 5) + kStepBias
constexpr int kGMax = 255;
constexpr float kQMax = 8388607.f;
constexpr int kZeroBand = -1, kNoBand = -2;       // L.base of a band below 2^-100, of a band at or above the cutoff
constexpr long kMaxSamples = (1L << 31) - 8;

enum { C_XOFF, C_N, C_YOFF, C_FRAMES, C_FOFF, C_K };
static_assert(C_XOFF == kRowOffset && C_N == kRowLength, "the plan opens with the shared row header");
enum { TOT_SAMPLES, TOT_FRAMES };

// floats of a frame size's table: roots of the M / 2-point transform, the DCT-IV twiddles (M / 2 complex each), the
// window (2M), T and R
constexpr long table_floats(int M) { return 2L * M + 2L * M + 2 * kSteps; }

struct Tables { const float2 *tw, *tw8; const float *win, *T, *R; };
__device__ __forceinline__ Tables tables_of(const float* t, int M) {
  return Tables{reinterpret_cast<const float2*>(t), reinterpret_cast<const float2*>(t + M), t + 2 * M, t + 4 * M,
                t + 4 * M + kSteps};
}

inline bool frame_ok(int M) { return M == 256 || M == 512 || M == 1024; }
inline int log2c_of(int M) { return M == 256 ? 7 : M == 512 ? 8 : 9; }
inline long frames_of(long n, int M) { return n > 0 ? (n + M - 1) / M + 1 : 0; }

// e_0 = 0, e_{b + 1} = min(M, e_b + max(4, 4 (e_b / 32))): every edge is a multiple of 4.  Returns the band count.
__host__ __device__ inline int band_edges(int M, int* e) {
  int nb = 0;
  e[0] = 0;
  while (e[nb] < M) {
    const int w = 4 * (e[nb] / 32) < 4 ? 4 : 4 * (e[nb] / 32);
    e[nb + 1] = e[nb] + w < M ? e[nb] + w : M;
    ++nb;
  }
  return nb;
}

inline int bands_below(int M, int k_c) {
  int e[kMaxBands + 1], c = 0;
  const int nb = band_edges(M, e);
  for (int b = 0; b < nb; ++b) c += e[b] < k_c;
  return c;
}

bool meta_ok(const long* hm, int n_rows, int M, long* totals2) {
  long s = 0, f = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * C_K;
    if (m[C_N] < 0 || m[C_N] > kMaxSamples || m[C_XOFF] < 0 || m[C_YOFF] < 0) return false;
    if (m[C_FRAMES] != frames_of(m[C_N], M) || m[C_FOFF] != f) return false;
    s += m[C_N]; f += m[C_FRAMES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_FRAMES] = f;
  return true;
}

int open_batch(int n_rows, int M, const long* host_meta, long* totals2) {
  return open_rows(n_rows, frame_ok(M) ? PE_OK : PE_E_UNSUPPORTED, host_meta,
                   [&] { return meta_ok(host_meta, n_rows, M, totals2); }, &totals2[TOT_SAMPLES]);
}

// ---- the stages, on one frame in LDS ---------------------------------------------------------------------------------
struct QuantLds {
  int edges[kMaxBands + 1], nb, nactive;          // per workgroup: the bands, those below the cutoff
  unsigned amax[kMaxBands];                       // per frame: bits of the band maximum
  int base[kMaxBands];                            // floor(2 s / 5) + kStepBias, kZeroBand or kNoBand
  int cost[kMaxBands], nz[kMaxBands], total;      // per pass
};

// the band of this thread's M / 256 consecutive bins (edges are multiples of 4, so they share one)
template <int M>
__device__ __forceinline__ int quant_setup(QuantLds& L, int k_c, int tid) {
  if (tid == 0) {
    L.nb = band_edges(M, L.edges);
    int c = 0;
    for (int b = 0; b < L.nb; ++b) c += L.edges[b] < k_c;
    L.nactive = c;
  }
  __syncthreads();
  const int k0 = tid * (M / kThreads);
  int b = 0;
  while (L.edges[b + 1] <= k0) ++b;
  return b;
}

// Frame f of a row, windowed: s_z[j] = w[j] x~[(f - 1) M + j]
template <int M>
__device__ __forceinline__ void load_frame(const float* __restrict__ xr, long n, long f, const float* __restrict__ win,
                                           float* s_z, int tid) {
  for (int j = tid; j < 2 * M; j += kThreads) {
    const long idx = (f - 1) * M + j;
    s_z[j] = idx >= 0 && idx < n ? xr[idx] * win[j] : 0.f;
  }
  __syncthreads();
}

// out[k] = sum over n < M of u(n) cos(pi / M (n + 1/2)(k + 1/2)): with v[n] = u(2n) + i u(M - 1 - 2n) and
// c = tw8 . FFT(tw8 . v), out[2k] = Re c[k] and out[M - 1 - 2k] = -Im c[k].  Every u is read before anything is
// written, so `out` may be where u reads.  Ends at a barrier.
template <int M, class In>
__device__ __forceinline__ void dct4(In&& u, float2* buf, const Tables& t, float* out, int tid) {
  constexpr int C = M / 2, LOG2C = M == 256 ? 7 : M == 512 ? 8 : 9;
  for (int n = tid; n < C; n += kThreads) buf[n] = cmul(make_float2(u(2 * n), u(M - 1 - 2 * n)), t.tw8[n]);
  __syncthreads();
  fft_lds<LOG2C, false, kThreads>(buf, t.tw, tid);
  for (int k = tid; k < C; k += kThreads) {
    const float2 c = cmul(buf[k], t.tw8[k]);
    out[2 * k] = c.x;
    out[M - 1 - 2 * k] = -c.y;
  }
  __syncthreads();
}

// The windowed 2M samples in s_z -> M coefficients in s_X.  With n = j + M / 2 the basis is odd about n = M - 1/2
// and about n = 2M - 1/2, which folds the 2M samples to M.
template <int M>
__device__ __forceinline__ void mdct_frame(const float* s_z, float2* buf, const Tables& t, float* s_X, int tid) {
  dct4<M>([&](int n) {
    return n < M / 2 ? -s_z[3 * M / 2 - 1 - n] - s_z[3 * M / 2 + n] : s_z[n - M / 2] - s_z[3 * M / 2 - 1 - n];
  }, buf, t, s_X, tid);
}

// M coefficients in s_X -> the windowed 2M samples of the frame at `fr` (global): (2 / M) w[j] sum_k X[k] cos(...)
template <int M>
__device__ __forceinline__ void imdct_frame(const float* s_X, float2* buf, const Tables& t, float* s_v,
                                            float* __restrict__ fr, int tid) {
  dct4<M>([&](int n) { return s_X[n]; }, buf, t, s_v, tid);
  for (int j = tid; j < 2 * M; j += kThreads) {
    const int n = j + M / 2;
    const float v = n < M ? s_v[n] : n < 2 * M ? -s_v[2 * M - 1 - n] : -s_v[n - 2 * M];
    fr[j] = (v * (2.f / M)) * t.win[j];
  }
  __syncthreads();
}

// floor(2 s / 5) + kStepBias with s = floor(4 log2 a) from the bits of a float32 a >= 2^-100: a = m 2^e, m in
// [0.5, 1), s = 4 (e - 1) + the count of 2^-0.75, 2^-0.5, 2^-0.25 (as float32) that are <= m
__device__ __forceinline__ int step_base(float a) {
  const unsigned bits = __float_as_uint(a);
  const int e = (int)(bits >> 23) - 126;
  const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f000000u);
  const int s = 4 * (e - 1) + (m >= 0.594603557501360533f) + (m >= 0.707106781186547524f) +
                (m >= 0.840896415253714543f);
  const int t = 2 * s;
  return (t >= 0 ? t / 5 : -((4 - t) / 5)) + kStepBias;
}

__device__ __forceinline__ int quant(float x, float r) {
  return (int)fminf(fmaxf(rintf(x * r), -kQMax), kQMax);
}

// The coefficients in s_X (bins >= k_c count as zero) -> their dequantised values in s_X; q (null: not kept), and
// the frame's g and bits in *g_out and *bits_out (by thread 0).  Ends at a barrier.
template <int M>
__device__ __forceinline__ void quantize_frame(float* s_X, QuantLds& L, int k_c, int budget, const Tables& t, int tid,
                                               int band, int* __restrict__ q_out, int* g_out, int* bits_out) {
  constexpr int NPT = M / kThreads;
  const int k0 = tid * NPT;
  float xv[NPT];
  unsigned mx = 0;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    xv[i] = k0 + i < k_c ? s_X[k0 + i] : 0.f;
    const unsigned b = __float_as_uint(xv[i]) & 0x7fffffffu;
    mx = b > mx ? b : mx;
  }
  if (tid < L.nb) L.amax[tid] = 0;
  __syncthreads();
  if (mx) atomicMax(&L.amax[band], mx);
  __syncthreads();
  if (tid < L.nb) {
    int base = kNoBand;
    if (L.edges[tid] < k_c) {
      const float a = __uint_as_float(L.amax[tid]);
      base = a >= 0x1p-100f ? step_base(a) : kZeroBand;
    }
    L.base[tid] = base;
  }
  __syncthreads();
  const int base = L.base[band];
  int qv[NPT];
#pragma unroll
  for (int i = 0; i < NPT; ++i) qv[i] = 0;

  // bits of the frame at gain g; qv = this thread's q.  A coefficient: 1 bit for 0, else gamma code plus sign; a band:
  // 1 bit if it is zero or quantises to zero, else 7 + its coefficients (those below the cutoff); the frame: 8 + bands.
  auto cost_at = [&](int g) {
    if (tid < L.nb) { L.cost[tid] = 0; L.nz[tid] = 0; }
    if (tid == 0) L.total = 0;
    __syncthreads();
    if (base >= 0) {
      const int idx = base + g < kSteps - 1 ? base + g : kSteps - 1;
      const float r = t.R[idx];
      int c = 0, nz = 0;
#pragma unroll
      for (int i = 0; i < NPT; ++i)
        if (k0 + i < k_c) {
          qv[i] = quant(xv[i], r);
          const int a = qv[i] < 0 ? -qv[i] : qv[i];
          c += a ? 2 * (31 - __clz(a + 1)) + 2 : 1;
          nz |= a;
        }
      atomicAdd(&L.cost[band], c);
      if (nz) atomicOr(&L.nz[band], 1);
    }
    __syncthreads();
    if (tid < L.nb && L.base[tid] != kNoBand) atomicAdd(&L.total, L.base[tid] >= 0 && L.nz[tid] ? 7 + L.cost[tid] : 1);
    __syncthreads();
    const int total = 8 + L.total;
    __syncthreads();
    return total;
  };

  int lo = 0, hi = kGMax;
  while (lo < hi) {                               // eight steps
    const int mid = (lo + hi) >> 1;
    if (cost_at(mid) <= budget) hi = mid; else lo = mid + 1;
  }
  int bits = cost_at(lo);
  const bool fits = bits <= budget;               // only g = 255 can miss: then the frame is all zero
  if (!fits) bits = 8 + L.nactive;
  const int idx = base + lo < kSteps - 1 ? base + lo : kSteps - 1;
  const float step = base >= 0 ? t.T[idx] : 0.f;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int q = fits && base >= 0 && k0 + i < k_c ? qv[i] : 0;
    s_X[k0 + i] = (float)q * step;
    if (q_out) q_out[k0 + i] = q;
  }
  if (tid == 0) {
    if (g_out) *g_out = lo;
    if (bits_out) *bits_out = bits;
  }
  __syncthreads();
}

// ---- kernels -------------------------------------------------------------------------------------------------------
// what: 1 mdct (x -> coefs), 2 imdct (coefs -> ws), 3 apply (x -> ws; g, bits optional)
template <int M, int WHAT>
__global__ __launch_bounds__(kThreads) void codec_frames_kernel(const float* __restrict__ x,
                                                                const long* __restrict__ meta,
                                                                const float* __restrict__ tables, int n_rows,
                                                                long frames, int k_c, int budget,
                                                                float* __restrict__ coefs, float* __restrict__ ws,
                                                                int* __restrict__ g_out, int* __restrict__ bits_out) {
  __shared__ float s_z[2 * M];
  __shared__ float2 s_buf[M / 2];
  __shared__ float s_X[M];
  __shared__ QuantLds L;
  const int tid = threadIdx.x;
  const Tables t = tables_of(tables, M);
  int band = 0;
  if constexpr (WHAT == 3) band = quant_setup<M>(L, k_c, tid);
  for (long g = blockIdx.x; g < frames; g += gridDim.x) {
    if constexpr (WHAT != 2) {
      const int row = find_row(meta, n_rows, C_K, C_FOFF, g);
      const long* m = meta + (long)row * C_K;
      load_frame<M>(x + m[C_XOFF], m[C_N], g - m[C_FOFF], t.win, s_z, tid);
      mdct_frame<M>(s_z, s_buf, t, s_X, tid);
    } else {
      for (int k = tid; k < M; k += kThreads) s_X[k] = coefs[g * M + k];
      __syncthreads();
    }
    if constexpr (WHAT == 1) {
      for (int k = tid; k < M; k += kThreads) coefs[g * M + k] = s_X[k];
      __syncthreads();
    } else {
      if constexpr (WHAT == 3)
        quantize_frame<M>(s_X, L, k_c, budget, t, tid, band, nullptr, g_out ? g_out + g : nullptr,
                          bits_out ? bits_out + g : nullptr);
      imdct_frame<M>(s_X, s_buf, t, s_z, ws + g * 2 * M, tid);
    }
  }
}

template <int M>
__global__ __launch_bounds__(kThreads) void codec_quantize_kernel(const float* __restrict__ coefs,
                                                                  const float* __restrict__ tables, long frames,
                                                                  int k_c, int budget, int* __restrict__ q,
                                                                  int* __restrict__ g_out, int* __restrict__ bits_out,
                                                                  float* __restrict__ deq) {
  __shared__ float s_X[M];
  __shared__ QuantLds L;
  const int tid = threadIdx.x;
  const Tables t = tables_of(tables, M);
  const int band = quant_setup<M>(L, k_c, tid);
  for (long g = blockIdx.x; g < frames; g += gridDim.x) {
    for (int k = tid; k < M; k += kThreads) s_X[k] = coefs[g * M + k];
    __syncthreads();
    quantize_frame<M>(s_X, L, k_c, budget, t, tid, band, q + g * M, g_out + g, bits_out + g);
    for (int k = tid; k < M; k += kThreads) deq[g * M + k] = s_X[k];
    __syncthreads();
  }
}

// Output block b of a row: the second half of its frame b plus the first half of its frame b + 1, in that order.
template <int M>
__global__ __launch_bounds__(kThreads) void codec_overlap_kernel(const float* __restrict__ ws,
                                                                 const long* __restrict__ meta, int n_rows, long frames,
                                                                 float* __restrict__ y) {
  for (long g = blockIdx.x; g < frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, C_K, C_FOFF, g);
    const long* m = meta + (long)row * C_K;
    const long n = m[C_N], b = g - m[C_FOFF];
    if (b + 1 >= m[C_FRAMES]) continue;           // the last frame opens no block
    const float* a = ws + g * 2 * M + M;
    const float* c = ws + (g + 1) * 2 * M;
    float* out = y + m[C_YOFF] + b * M;
    for (int r = threadIdx.x; r < M; r += kThreads)
      if (b * M + r < n) out[r] = a[r] + c[r];
  }
}

// G.711 mu-law, encoder and decoder back to back, on the 16-bit value p = rint(32768 x) clamped
__device__ __forceinline__ float mulaw(float x) {
  const int p = (int)fminf(fmaxf(rintf(x * 32768.f), -32768.f), 32767.f);
  const int mag = p < 0 ? -p : p;
  const int m = (mag < 32635 ? mag : 32635) + 132;
  const int e = 31 - __clz(m) - 7;
  const int mant = (m >> (e + 3)) & 15;
  const int v = (((mant << 3) + 132) << e) - 132;
  return (float)(p < 0 ? -v : p > 0 ? v : 0) / 32768.f;
}

__global__ __launch_bounds__(kThreads) void codec_mulaw_kernel(const float* __restrict__ x,
                                                               const long* __restrict__ meta, int n_rows, long frames,
                                                               int M, float* __restrict__ y) {
  for (long g = blockIdx.x; g < frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, C_K, C_FOFF, g);
    const long* m = meta + (long)row * C_K;
    const long n = m[C_N], first = (g - m[C_FOFF]) * M;
    const float* xr = x + m[C_XOFF] + first;
    float* yr = y + m[C_YOFF] + first;
    for (int r = threadIdx.x; r < M; r += kThreads)
      if (first + r < n) yr[r] = mulaw(xr[r]);
  }
}

bool quantizer_ok(int M, int k_c, int budget) {
  return k_c >= 1 && k_c <= M && budget >= 8 + bands_below(M, k_c);
}

// calls fn(std::integral_constant<int, M>) for the frame size (open_batch has refused any other)
template <class Fn>
int with_frame(int M, Fn&& fn) {
  return with_log2<7, 9>(log2c_of(M),
                         [&](auto lg) { return fn(std::integral_constant<int, 2 << decltype(lg)::value>{}); });
}

template <int WHAT>
int launch_frames(int M, const float* x, const long* meta, const float* tables, int n_rows, long frames, int k_c,
                  int budget, float* coefs, float* ws, int* g, int* bits, void* stream) {
  return with_frame(M, [&](auto mc) {
    constexpr int kM = decltype(mc)::value;
    hipLaunchKernelGGL((codec_frames_kernel<kM, WHAT>), dim3(grid_of(frames)), dim3(kThreads), 0, pe_stream(stream), x,
                       meta, tables, n_rows, frames, k_c, budget, coefs, ws, g, bits);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

int launch_overlap(int M, const float* ws, const long* meta, int n_rows, long frames, float* y, void* stream) {
  return with_frame(M, [&](auto mc) {
    constexpr int kM = decltype(mc)::value;
    hipLaunchKernelGGL((codec_overlap_kernel<kM>), dim3(grid_of(frames)), dim3(kThreads), 0, pe_stream(stream), ws,
                       meta, n_rows, frames, y);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

}  // namespace

extern "C" int pe_codec_plan_fields(void) { return C_K; }

extern "C" int pe_codec_bands(int frame, int* edges, int n_edges) {
  if (!frame_ok(frame) || !edges || n_edges < kMaxBands + 1) return PE_E_ARG;
  return band_edges(frame, edges);
}

/* Host-only layout; see include/pitchextractor_hip.h. */
extern "C" int pe_codec_plan(int n_rows, int frame, const long* n, const long* x_off, const long* y_off, long* consts4,
                             long* meta, long* totals2) {
  if (!consts4 || !totals2 || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (!frame_ok(frame)) return PE_E_UNSUPPORTED;
  if (n_rows > 0 && (!n || !x_off || !y_off || !meta)) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (n[r] < 0 || n[r] > kMaxSamples || x_off[r] < 0 || y_off[r] < 0) return PE_E_ARG;
  int e[kMaxBands + 1];
  consts4[0] = frame; consts4[1] = table_floats(frame); consts4[2] = band_edges(frame, e); consts4[3] = kSteps;
  long s = 0, f = 0;
  for (int r = 0; r < n_rows; ++r) {
    long* m = meta + (long)r * C_K;
    m[C_XOFF] = x_off[r]; m[C_N] = n[r]; m[C_YOFF] = y_off[r];
    m[C_FRAMES] = frames_of(n[r], frame); m[C_FOFF] = f;
    s += n[r]; f += m[C_FRAMES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_FRAMES] = f;
  return PE_OK;
}

extern "C" size_t pe_codec_workspace_bytes(int frame, long frames) {
  return frame_ok(frame) && frames > 0 ? (size_t)frames * 2 * frame * sizeof(float) : 0;
}

extern "C" int pe_codec_mdct(const float* x, const long* meta, const long* host_meta, int n_rows, int frame,
                             const float* tables, long n_table, float* coefs, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, frame, host_meta, tot));
  if (!x || !meta || !tables || !coefs || n_table != table_floats(frame)) return PE_E_ARG;
  return launch_frames<1>(frame, x, meta, tables, n_rows, tot[TOT_FRAMES], 0, 0, coefs, nullptr, nullptr, nullptr,
                          stream);
}

extern "C" int pe_codec_quantize(const float* coefs, long frames, int frame, int k_c, int budget, const float* tables,
                                 long n_table, int* q, int* g, int* bits, float* dequantised, void* stream) {
  if (!frame_ok(frame)) return PE_E_UNSUPPORTED;
  if (frames < 0 || !quantizer_ok(frame, k_c, budget)) return PE_E_ARG;
  if (frames == 0) return PE_OK;
  if (!coefs || !tables || !q || !g || !bits || !dequantised || n_table != table_floats(frame)) return PE_E_ARG;
  return with_frame(frame, [&](auto mc) {
    constexpr int kM = decltype(mc)::value;
    hipLaunchKernelGGL((codec_quantize_kernel<kM>), dim3(grid_of(frames)), dim3(kThreads), 0, pe_stream(stream), coefs,
                       tables, frames, k_c, budget, q, g, bits, dequantised);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

extern "C" int pe_codec_imdct(const float* coefs, const long* meta, const long* host_meta, int n_rows, int frame,
                              const float* tables, long n_table, float* y, void* workspace, size_t workspace_bytes,
                              void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, frame, host_meta, tot));
  if (!coefs || !meta || !tables || !y || n_table != table_floats(frame)) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_codec_workspace_bytes(frame, tot[TOT_FRAMES])) return PE_E_WORKSPACE;
  float* ws = static_cast<float*>(workspace);
  const int st = launch_frames<2>(frame, nullptr, meta, tables, n_rows, tot[TOT_FRAMES], 0, 0,
                                  const_cast<float*>(coefs), ws, nullptr, nullptr, stream);
  return st != PE_OK ? st : launch_overlap(frame, ws, meta, n_rows, tot[TOT_FRAMES], y, stream);
}

extern "C" int pe_codec_apply(const float* x, const long* meta, const long* host_meta, int n_rows, int frame, int k_c,
                              int budget, const float* tables, long n_table, float* y, int* g, int* bits,
                              void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2];
  const int st0 = open_batch(n_rows, frame, host_meta, tot);
  if (st0 != PE_OK && st0 != kNothing) return st0;
  if (!quantizer_ok(frame, k_c, budget)) return PE_E_ARG;
  if (st0 == kNothing) return PE_OK;
  if (!x || !meta || !tables || !y || n_table != table_floats(frame)) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_codec_workspace_bytes(frame, tot[TOT_FRAMES])) return PE_E_WORKSPACE;
  float* ws = static_cast<float*>(workspace);
  const int st = launch_frames<3>(frame, x, meta, tables, n_rows, tot[TOT_FRAMES], k_c, budget, nullptr, ws, g, bits,
                                  stream);
  return st != PE_OK ? st : launch_overlap(frame, ws, meta, n_rows, tot[TOT_FRAMES], y, stream);
}

extern "C" int pe_codec_mulaw(const float* x, const long* meta, const long* host_meta, int n_rows, int frame, float* y,
                              void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, frame, host_meta, tot));
  if (!x || !meta || !y) return PE_E_ARG;
  hipLaunchKernelGGL(codec_mulaw_kernel, dim3(grid_of(tot[TOT_FRAMES])), dim3(kThreads), 0, pe_stream(stream), x, meta,
                     n_rows, tot[TOT_FRAMES], frame, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
