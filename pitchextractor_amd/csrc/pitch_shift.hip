// Pitch-shift augmentation on the GPU: librosa.effects.pitch_shift(y, sr, n_steps, res_type) with its defaults
// (librosa 0.10: STFT n_fft 2048 / hop 512 / periodic Hann / centre zero padding -> phase vocoder at
// rate = 2^(-n_steps/12) -> iSTFT to round(N / rate) samples -> resampy band-limited sinc resampling back to N
// samples), as the reference's synthetic-data generator calls it (meldataset.py:324-517).
//
// Ragged batches: every row has its own length, semitone, gain and output window.  pe_pitch_shift_plan (host only)
// lays the batch out; the four stages then walk flat work indices and find their row by a binary search over the
// plan's prefix offsets, so a 5-minute file next to 2-second ones costs only its own work.  Only the prefix of a row
// that the kept output window depends on is computed: the phase vocoder must walk every column before the window
// (its phase is a running sum), nothing after it is needed.
//
//   1. STFT: one wave per frame; the 2048 real samples are packed as 1024 complex points and run through five radix-4
//      Stockham passes in LDS, then split into the 1025 bins of the real transform -- in fp64, rounded at the store
//      (the inverse transform of stage 3 is fft_lds of dsp.h in fp32).
//   2. Phase vocoder: one lane per (row, bin) walks the output columns.  The phase advance of bin k per column is
//      k * pi / 2 exactly, so the accumulated phase is carried as an integer quarter-turn count (t * k) mod 4 plus an
//      fp64 residual reduced to [-pi, pi) every column; a plain fp32 running phase grows to 1e5-1e6 rad on long files.
//   3. iSTFT: one wave per column (inverse real FFT x window), then an overlap-add in gather form -- every output
//      sample reads its <= 4 frames, no atomics -- divided by the window sum-square where that exceeds FLT_MIN.
//   4. Resampler: one thread per output sample of the kept window; the read position j / r is formed in fp64 (fp32
//      is 0.06 samples off at 1e6); the filter table (host-built, 128 KB / 32 KB) stays in L2.  At ratio 1 exactly
//      (n_steps = 0) the sample is copied, as librosa's resample hands its input back when the rates are equal.
//      Gain, optional noise and the write into the caller's batch row are the epilogue.
#include <float.h>
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kN = 2048;          // n_fft
constexpr int kHop = 512;
constexpr int kBins = kN / 2 + 1;
constexpr int kLog2C = 10;
constexpr int kC = 1 << kLog2C;    // complex FFT length kN / 2; one wave per transform: fft_lds<kLog2C, INV, 64>
static_assert(2 * kC == kN, "the real frame is packed as kN / 2 complex points");
constexpr int kP = 512;           // resampy table precision 2^9
constexpr double kPiD = 3.14159265358979323846;

// per-row plan fields (int64); see pe_pitch_shift_plan
enum {
  M_N, M_XOFF, M_FUSE, M_FOFF, M_CLO, M_CHI, M_COFF, M_M, M_NOLA, M_SLO, M_SHI, M_SOFF, M_NRES, M_JLO, M_JCNT,
  M_JOFF, M_OOFF, M_NCOLS, M_K
};

// block-shared tables: 1024th roots of unity (forward sign), 2048th roots for the real split, Hann window
__device__ void init_tables(float2* s_tw, float2* s_tr, float* s_win) {
  for (int m = threadIdx.x; m < kC; m += blockDim.x) {
    double s, c;
    sincospi(-2.0 * m / kC, &s, &c);
    s_tw[m] = make_float2((float)c, (float)s);
  }
  for (int m = threadIdx.x; m < kBins; m += blockDim.x) {
    double s, c;
    sincospi(-2.0 * m / kN, &s, &c);
    s_tr[m] = make_float2((float)c, (float)s);
  }
  if (s_win)
    for (int i = threadIdx.x; i < kN; i += blockDim.x) s_win[i] = (float)(0.5 - 0.5 * cospi(2.0 * i / kN));
}

// ---- 1. STFT ---------------------------------------------------------------------------------------------------------
// The forward transform runs in fp64 and rounds once, at the store.  A float32 transform leaves a noise floor under
// every bin of a frame (the packed radix-4 passes: 4.5e-9 rms of the largest bin, three times numpy's float32 FFT); the
// phase vocoder reads the phase of bins that rise out of that floor on a glide, and end to end the stage alone cost
// 2.3 times the error of a float32 librosa at an octave.  Same algorithm as fft_lds (dsp.h: radix-4 Stockham passes in
// place, one wave per buffer), on double2, with one table: the 2048th roots 0 .. 1024, which also hold the 1024th roots
// (every other one, mirrored past the half turn) and the Hann window (0.5 - 0.5 cos).
constexpr int kStftWaves = 2;                             // 2 x 16 KB of buffers + 16 KB of roots per workgroup

__device__ __forceinline__ double2 dmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// exp(-2 pi i j / 2048), j in [0, 2048)
__device__ __forceinline__ double2 root2048(const double2* tr, int j) {
  if (j <= kC) return tr[j];
  const double2 w = tr[kN - j];
  return make_double2(w.x, -w.y);
}

__device__ __forceinline__ void fft1024_fwd_f64(double2* buf, const double2* tr, int lane) {
  constexpr int NB = kC / 4 / 64;
#pragma unroll
  for (int p = 0; p < kLog2C / 2; ++p) {
    const int ns = 1 << (2 * p), shift = kLog2C - 2 - 2 * p;
    double2 v[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[b][r] = buf[lane + 64 * b + (kC / 4) * r];
    wave_lds_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int j = lane + 64 * b, k = j & (ns - 1);
#pragma unroll
      for (int r = 1; r < 4; ++r) v[b][r] = dmul(v[b][r], root2048(tr, 2 * ((r * k) << shift)));
      const double2 t0 = make_double2(v[b][0].x + v[b][2].x, v[b][0].y + v[b][2].y);
      const double2 t1 = make_double2(v[b][0].x - v[b][2].x, v[b][0].y - v[b][2].y);
      const double2 t2 = make_double2(v[b][1].x + v[b][3].x, v[b][1].y + v[b][3].y);
      const double2 t3 = make_double2(v[b][1].y - v[b][3].y, v[b][3].x - v[b][1].x);      // (v1 - v3) * -i
      const int o = ((j >> (2 * p)) << (2 * p + 2)) + k;
      buf[o] = make_double2(t0.x + t2.x, t0.y + t2.y);
      buf[o + ns] = make_double2(t1.x + t3.x, t1.y + t3.y);
      buf[o + 2 * ns] = make_double2(t0.x - t2.x, t0.y - t2.y);
      buf[o + 3 * ns] = make_double2(t1.x - t3.x, t1.y - t3.y);
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(64 * kStftWaves) void ps_stft_kernel(const float* __restrict__ x,
                                                                  const long* __restrict__ meta, int n_rows,
                                                                  long total, float2* __restrict__ spec) {
  __shared__ double2 s_tr[kBins];
  __shared__ double2 s_buf[kStftWaves][kC];
  for (int m = threadIdx.x; m < kBins; m += blockDim.x) {
    double s, c;
    sincospi(-2.0 * m / kN, &s, &c);
    s_tr[m] = make_double2(c, s);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double2* buf = s_buf[wv];
  auto hann = [&](int i) { return 0.5 - 0.5 * s_tr[i <= kC ? i : kN - i].x; };
  for (long g = (long)blockIdx.x * kStftWaves + wv; g < total; g += (long)gridDim.x * kStftWaves) {
    const int row = find_row(meta, n_rows, M_K, M_FOFF, g);
    const long* m = meta + (long)row * M_K;
    const long f = g - m[M_FOFF], n = m[M_N];
    const float* xr = x + m[M_XOFF];
    const long base = f * kHop - kN / 2;                  // centre=True: frame f starts 1024 samples early, zero padded
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = 2 * (lane + 64 * q);
      const long a = base + i;
      const double v0 = (a >= 0 && a < n) ? (double)xr[a] : 0.0;
      const double v1 = (a + 1 >= 0 && a + 1 < n) ? (double)xr[a + 1] : 0.0;
      buf[i >> 1] = make_double2(v0 * hann(i), v1 * hann(i + 1));
    }
    wave_lds_sync();
    fft1024_fwd_f64(buf, s_tr, lane);
    float2* out = spec + g * kBins;
#pragma unroll
    for (int q = 0; q < 17; ++q) {
      const int k = lane + 64 * q;
      if (k > kC) break;
      // bin k of the real transform from the packed one (real_fft_bin of dsp.h, in fp64): e + w o
      const double2 zk = buf[k & (kC - 1)], zc = buf[(kC - k) & (kC - 1)];
      const double2 e = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y - zc.y));
      const double2 o = make_double2(0.5 * (zk.y + zc.y), -0.5 * (zk.x - zc.x));
      const double2 t = dmul(s_tr[k], o);
      out[k] = make_float2((float)(e.x + t.x), (float)(e.y + t.y));
    }
    wave_lds_sync();                                      // buffer reads done before the next frame's writes
  }
}

// ---- 2. phase vocoder ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wrap_pi(double p) {     // p - 2 pi round(p / 2 pi), round half to even like numpy
  return fma(-rint(p * (0.5 / kPiD)), 2.0 * kPiD, p);
}

__global__ __launch_bounds__(256) void ps_vocoder_kernel(const float2* __restrict__ spec, const long* __restrict__ meta,
                                                         const double* __restrict__ ratios, float2* __restrict__ cols) {
  const int row = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= kBins) return;
  const long* m = meta + (long)row * M_K;
  const long c_hi = m[M_CHI], c_lo = m[M_CLO], f_use = m[M_FUSE];
  if (c_hi <= 0) return;
  const double rate = ratios[2 * row];
  const float2* D = spec + m[M_FOFF] * kBins + k;
  float2* out = cols + m[M_COFF] * kBins + k;
  const float2 zero = make_float2(0.f, 0.f);
  // x + 0 turns -0 into +0: the phase of an exactly silent bin is then atan2(+0, +0) = 0, as numpy's spectrum of
  // silence gives; a -0 from the FFT's sign flips would put pi into the running phase of every later column
  auto ld = [&](long f) { const float2 v = D[f * kBins]; return make_float2(v.x + 0.f, v.y + 0.f); };
  // The residual and its increments are fp64: float(k pi / 2) is off by up to 2.4e-7 rad, and subtracting it every
  // column walked the fp32 residual away from float64 at that rate (8e-4 rad after 8192 columns, a 3-minute file).
  const double adv = (double)(k & 3) * (0.5 * kPiD);      // k pi / 2 mod 2 pi
  const float2 d0 = ld(0);
  double rho = (double)atan2f(d0.y, d0.x);                // phase residual in [-pi, pi]
  int q = 0;                                              // quarter turns (t k) mod 4
  long i0 = 0;
  float2 A = d0, B = f_use > 1 ? ld(1) : zero;
  for (long t = 0; t < c_hi; ++t) {
    const double st = (double)t * rate;
    const float alpha = (float)(st - (double)i0);
    // next column pair, issued before this column's arithmetic
    const long i1 = (long)((double)(t + 1) * rate);
    const float2 nA = (t + 1 < c_hi && i1 < f_use) ? ld(i1) : zero;
    const float2 nB = (t + 1 < c_hi && i1 + 1 < f_use) ? ld(i1 + 1) : zero;
    const float ma = sqrtf(A.x * A.x + A.y * A.y), mb = sqrtf(B.x * B.x + B.y * B.y);
    const float mag = (1.f - alpha) * ma + alpha * mb;
    if (t >= c_lo) {
      float s, c;
      sincosf((float)rho, &s, &c);
      float2 ph = make_float2(c, s);
      if (q & 1) ph = make_float2(-ph.y, ph.x);           // * i
      if (q & 2) ph = make_float2(-ph.x, -ph.y);          // * -1
      out[(t - c_lo) * kBins] = make_float2(mag * ph.x, mag * ph.y);
    }
    rho += wrap_pi((double)atan2f(B.y, B.x) - (double)atan2f(A.y, A.x) - adv);
    if (rho >= kPiD) rho -= 2.0 * kPiD;
    else if (rho < -kPiD) rho += 2.0 * kPiD;
    q = (q + k) & 3;
    A = nA; B = nB; i0 = i1;
  }
}

// ---- 3. iSTFT ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ps_irfft_kernel(const float2* __restrict__ cols, const long* __restrict__ meta,
                                                       int n_rows, long total, float* __restrict__ frames) {
  __shared__ float2 s_tw[kC];
  __shared__ float2 s_tr[kBins];
  __shared__ float s_win[kN];
  __shared__ float2 s_buf[4][kC];
  init_tables(s_tw, s_tr, s_win);
  __syncthreads();
  (void)meta; (void)n_rows;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float2* buf = s_buf[wv];
  for (long g = (long)blockIdx.x * 4 + wv; g < total; g += (long)gridDim.x * 4) {
    const float2* X = cols + g * kBins;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int k = lane + 64 * q;
      float2 xk = X[k], xc = conj2(X[kC - k]);
      if (k == 0) { xk.y = 0.f; xc.y = 0.f; }               // numpy irfft drops Im of the DC and Nyquist bins
      buf[k] = real_fft_pack(xk, xc, s_tr[k]);              // E + i O
    }
    wave_lds_sync();
    fft_lds<kLog2C, true, 64>(buf, s_tw, lane);
    float* out = frames + g * kN;
    constexpr float inv = 1.f / kC;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = lane + 64 * q;
      const float2 z = buf[n];
      *reinterpret_cast<float2*>(out + 2 * n) = make_float2(z.x * inv * s_win[2 * n], z.y * inv * s_win[2 * n + 1]);
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(256) void ps_ola_kernel(const float* __restrict__ frames, const long* __restrict__ meta,
                                                     int n_rows, long total, float* __restrict__ stretched) {
  __shared__ float s_w2[kN];
  for (int i = threadIdx.x; i < kN; i += 256) {
    const double w = 0.5 - 0.5 * cospi(2.0 * i / kN);
    s_w2[i] = (float)(w * w);
  }
  __syncthreads();
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const int row = find_row(meta, n_rows, M_K, M_SOFF, g);
    const long* m = meta + (long)row * M_K;
    const long p = m[M_SLO] + (g - m[M_SOFF]) + kN / 2;    // position in the overlap-add buffer (centre dropped)
    const long n_ola = m[M_NOLA], c_lo = m[M_CLO], c_hi = m[M_CHI];
    float acc = 0.f, wss = 0.f;
    if (p < kN + kHop * (n_ola - 1)) {
      const long t_lo = p < kN ? 0 : (p - kN) / kHop + 1;
      const long t_hi = min(n_ola - 1, p / kHop);
      for (long t = t_lo; t <= t_hi; ++t) {
        const int i = (int)(p - kHop * t);
        if (t >= c_lo && t < c_hi) acc += frames[(m[M_COFF] + t - c_lo) * kN + i];
        wss += s_w2[i];
      }
    }
    stretched[g] = wss > FLT_MIN ? acc / wss : acc;
  }
}

// ---- 4. resampler + epilogue ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ps_resample_kernel(const float* __restrict__ st, const long* __restrict__ meta,
                                                          const double* __restrict__ ratios,
                                                          const float* __restrict__ win, const float* __restrict__ dwin,
                                                          int nwin, const float* __restrict__ gains,
                                                          const float* __restrict__ noise, int n_rows, long total,
                                                          float* __restrict__ out) {
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const int row = find_row(meta, n_rows, M_K, M_JOFF, g);
    const long* m = meta + (long)row * M_K;
    const long i = g - m[M_JOFF], j = m[M_JLO] + i;
    float v = 0.f;
    const double r = ratios[2 * row + 1];
    const long s_lo = m[M_SLO], s_hi = m[M_SHI];
    const float* x = st + m[M_SOFF] - s_lo;                   // x[s] for s in [s_lo, s_hi)
    if (r == 1.0) {
      // n_steps = 0: librosa's resample returns its input when the two rates are equal, no low-pass is applied
      if (j < m[M_NRES] && j >= s_lo && j < s_hi) v = x[j];
    } else if (j < m[M_NRES]) {
      const double scale = r < 1.0 ? r : 1.0;
      const long step = (long)(scale * kP);
      const long M = m[M_M];
      const double T = (double)j / r;
      const long n = (long)T;
      double frac = scale * (T - (double)n);
      double idx_f = frac * kP;
      long off = (long)idx_f;
      float eta = (float)(idx_f - (double)off);
      const long i_max = min(n + 1, (nwin - off) / step);
      for (long a = 0; a < i_max; ++a) {
        const long s = n - a, w = off + a * step;
        if (s >= s_lo && s < s_hi) v = fmaf(fmaf(eta, dwin[w], win[w]), x[s], v);
      }
      frac = scale - frac;
      idx_f = frac * kP;
      off = (long)idx_f;
      eta = (float)(idx_f - (double)off);
      const long k_max = min(M - n - 1, (nwin - off) / step);
      for (long a = 0; a < k_max; ++a) {
        const long s = n + 1 + a, w = off + a * step;
        if (s >= s_lo && s < s_hi) v = fmaf(fmaf(eta, dwin[w], win[w]), x[s], v);
      }
      v *= (float)scale;                                     // resampy scales the table by the ratio when it is < 1
    }
    float y = v * gains[row];
    if (noise) y += noise[g];
    out[m[M_OOFF] + i] = y;
  }
}

constexpr int kZeros[2] = {64, 16};                          // kaiser_best, kaiser_fast zero crossings

}  // namespace

/* Host-only batch layout; see include/pitchextractor_hip.h. */
extern "C" int pe_pitch_shift_plan(int n_rows, const long* n, const float* n_steps, const long* x_off,
                                   const long* j_lo, const long* j_cnt, const long* out_row, long out_stride, int sr,
                                   int n_fft, int hop, int res_type, long* meta, double* ratios, long* totals) {
  if (n_fft != kN || hop != kHop) return PE_E_UNSUPPORTED;
  if (n_rows < 0 || n_rows > kMaxRows || sr <= 0 || res_type < 0 || res_type > 1 || !totals) return PE_E_ARG;
  if (n_rows > 0 && (!n || !n_steps || !x_off || !j_lo || !j_cnt || !out_row || !meta || !ratios)) return PE_E_ARG;
  const long nwin = (long)kZeros[res_type] * kP + 1;
  long f_tot = 0, c_tot = 0, s_tot = 0, j_tot = 0;
  for (int r = 0; r < n_rows; ++r) {
    const double s = (double)n_steps[r];
    if (n[r] < 1 || n[r] > (1L << 31) || !isfinite(s) || fabs(s) > 24.0 || x_off[r] < 0 || j_lo[r] < 0 ||
        j_cnt[r] < 0 || j_lo[r] + j_cnt[r] > n[r] || out_row[r] < 0 || out_stride < j_cnt[r])
      return PE_E_ARG;
    const long N = n[r];
    const double rate = pow(2.0, -s / 12.0);                  // librosa: 2.0 ** (-n_steps / 12)
    const double ratio = (double)sr / ((double)sr / rate);    // resampy: sr_new / sr_orig with sr_orig = sr / rate
    const long F = 1 + N / kHop;
    const long n_cols = (long)ceil((double)F / rate);         // len(np.arange(0, F, rate))
    const long M = (long)nearbyint((double)N / rate);         // int(round(N / rate)), half to even
    const long n_ola = min(n_cols, (M + kN + kHop - 1) / kHop);
    const long n_res = (long)((double)M * ratio);
    const long j_end = min(j_lo[r] + j_cnt[r], n_res);
    long s_lo = 0, s_hi = 0, c_lo = 0, c_hi = 0, f_use = 0;
    if (j_end > j_lo[r]) {
      const double scale = ratio < 1.0 ? ratio : 1.0;
      const long taps = nwin / (long)(scale * kP) + 1;
      s_lo = max(0L, (long)((double)j_lo[r] / ratio) - taps);
      s_hi = min(M, (long)((double)(j_end - 1) / ratio) + 2 + taps);
      if (s_hi < s_lo) s_hi = s_lo;
    }
    if (s_hi > s_lo) {
      c_lo = s_lo < kN / 2 ? 0 : (s_lo - kN / 2) / kHop + 1;
      c_hi = min(n_ola, (s_hi - 1 + kN / 2) / kHop + 1);
      if (c_lo > c_hi) c_lo = c_hi;
      if (c_hi > 0) f_use = min(F, (long)((double)(c_hi - 1) * rate) + 2);
    }
    long* m = meta + (long)r * M_K;
    m[M_N] = N; m[M_XOFF] = x_off[r]; m[M_FUSE] = f_use; m[M_FOFF] = f_tot; m[M_CLO] = c_lo; m[M_CHI] = c_hi;
    m[M_COFF] = c_tot; m[M_M] = M; m[M_NOLA] = n_ola; m[M_SLO] = s_lo; m[M_SHI] = s_hi; m[M_SOFF] = s_tot;
    m[M_NRES] = n_res; m[M_JLO] = j_lo[r]; m[M_JCNT] = j_cnt[r]; m[M_JOFF] = j_tot;
    m[M_OOFF] = out_row[r] * out_stride; m[M_NCOLS] = n_cols;
    ratios[2 * r] = rate;
    ratios[2 * r + 1] = ratio;
    f_tot += f_use; c_tot += c_hi - c_lo; s_tot += s_hi - s_lo; j_tot += j_cnt[r];
  }
  totals[0] = f_tot; totals[1] = c_tot; totals[2] = s_tot; totals[3] = j_tot;
  return PE_OK;
}

extern "C" int pe_pitch_shift_plan_fields(void) { return M_K; }

extern "C" int pe_pitch_shift_stft(const float* x, const long* meta, int n_rows, long n_frames, float* spec,
                                   void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_frames < 0) return PE_E_ARG;
  if (n_frames == 0 || n_rows == 0) return PE_OK;
  if (!x || !meta || !spec) return PE_E_ARG;
  hipLaunchKernelGGL(ps_stft_kernel, dim3(grid_for(n_frames, kStftWaves, 1024)), dim3(64 * kStftWaves), 0,
                     pe_stream(stream), x, meta, n_rows, n_frames, reinterpret_cast<float2*>(spec));
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_pitch_shift_vocoder(const float* spec, const long* meta, const double* ratios, int n_rows,
                                      long n_cols, float* cols, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_cols < 0) return PE_E_ARG;
  if (n_cols == 0 || n_rows == 0) return PE_OK;
  if (!spec || !meta || !ratios || !cols) return PE_E_ARG;
  hipLaunchKernelGGL(ps_vocoder_kernel, dim3(pe_cdiv(kBins, 256), n_rows), dim3(256), 0, pe_stream(stream),
                     reinterpret_cast<const float2*>(spec), meta, ratios, reinterpret_cast<float2*>(cols));
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_pitch_shift_istft(const float* cols, const long* meta, int n_rows, long n_cols, long n_samples,
                                    float* frames, float* stretched, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_cols < 0 || n_samples < 0) return PE_E_ARG;
  if (n_samples == 0 || n_rows == 0) return PE_OK;
  if (!meta || !stretched || (n_cols > 0 && (!cols || !frames))) return PE_E_ARG;
  if (n_cols > 0) {
    hipLaunchKernelGGL(ps_irfft_kernel, dim3(grid_for(n_cols, 4, 2048)), dim3(256), 0, pe_stream(stream),
                       reinterpret_cast<const float2*>(cols), meta, n_rows, n_cols, frames);
    PE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ps_ola_kernel, dim3(grid_for(n_samples, 256, 4096)), dim3(256), 0, pe_stream(stream), frames,
                     meta, n_rows, n_samples, stretched);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_pitch_shift_resample(const float* stretched, const long* meta, const double* ratios,
                                       const float* table, int res_type, const float* gains, const float* noise,
                                       int n_rows, long n_out, float* out, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_out < 0 || res_type < 0 || res_type > 1) return PE_E_ARG;
  if (n_out == 0 || n_rows == 0) return PE_OK;
  if (!stretched || !meta || !ratios || !table || !gains || !out) return PE_E_ARG;
  const int nwin = kZeros[res_type] * kP + 1;
  hipLaunchKernelGGL(ps_resample_kernel, dim3(grid_for(n_out, 256, 8192)), dim3(256), 0, pe_stream(stream), stretched,
                     meta, ratios, table, table + nwin, nwin, gains, noise, n_rows, n_out, out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
