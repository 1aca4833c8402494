// F0 labels on the GPU: WORLD's DIO followed by StoneMask (M. Morise, H. Kawahara, H. Katayose, "Fast and reliable F0
// estimation method based on the period extraction of vocal fold vibration of singing voice and speech", AES 35th
// Int. Conf., 2009; WORLD's `dio` / `stonemask` with pyworld's defaults: no decimation), the algorithm behind the
// reference's `pyworld` backend with `algorithm: dio`.  Pinned by the float64 restatement in tests/dio_ref.py; parity
// with pyworld's own binary is unpinned.
//
// Ragged batches: pe_f0_dio_plan (host only) derives the constants and lays the rows out by prefix offsets of their
// frames, samples, overlap-save blocks and event chunks.  Every stage has its own entry point:
//   bands:      one workgroup per (row, block).  The block of x - mean is transformed once (packed real FFT in LDS,
//               fft_lds); per band the spectrum is multiplied by the band's filter spectrum (low-cut x Nuttall low-pass,
//               delay compensated, built on the host in float64) and transformed back: overlap-save.
//   events:     zero crossings of the band signal, its negation, its first difference and the negated difference, in
//               order: count per chunk, prefix per (row, band, kind), scatter.  A fine edge is an integer sample index
//               and a float32 fraction, never a float32 absolute position.
//   candidates: one thread per (row, frame, band): the four interval tracks interpolated at the frame time, their mean
//               and spread, the range tests; then the band of the lowest score per frame.
//   fix:        FixF0Contour steps 1-4, one wave per row (a short sequential pass).
//   stonemask:  one workgroup per voiced frame: Blackman window and its centred difference as the real and the
//               imaginary input of one complex FFT whose size depends on the frame's F0.
// No atomics, no cross-workgroup communication inside a launch: a row's result does not depend on the batch around it.
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBands = 16;
constexpr int kChunk = 2048;              // samples of a band signal per event workgroup (4 waves x 8 x 64)
constexpr int kKinds = 4;
constexpr double kLowCut = 50.0;
constexpr float kRejected = 100000.f;
constexpr int kSmMaxLog2 = 12;            // StoneMask transforms: 128 .. 4096 points
constexpr int kSmMinLog2 = 7;

enum { D_XOFF, D_N, D_FRAMES, D_FOFF, D_SOFF, D_BLOCKS, D_BOFF, D_EOFF, D_CHUNKS, D_COFF, D_K };
static_assert(D_XOFF == kRowOffset && D_N == kRowLength, "the plan opens with the shared row header");

struct DioConsts {
  int sr, hop, bands, nfft, log2c, taps, step, lead, vrm, cut;
  int half[kMaxBands];
  float boundary[kMaxBands];
  double frame_period, boundary_d[kMaxBands];
  float floor_f, ceil_f, allowed;
  double floor_d;
};

double round_half_away(double v) { return v < 0.0 ? -floor(-v + 0.5) : floor(v + 0.5); }

// StoneMask's largest transform is the one of the lowest F0 a contour may hold, f0_min: does it fit 2^kSmMaxLog2 points?
bool stonemask_fits(int sr, double f0_min) {
#pragma clang fp contract(off)
  const double lowest = f0_min > 40.0 ? f0_min : 40.0;
  const int hw = (int)(1.5 * (double)sr / lowest + 1.0);
  int lg = 0;
  while ((2 << lg) <= 2 * hw + 1) ++lg;
  return 2 + lg <= kSmMaxLog2;
}

// step 1 of the algorithm for (sr, hop, config4 = {f0_floor, f0_ceil, channels_in_octave, allowed_range})
int derive(int sr, int hop, const double* cfg, DioConsts* k) {
#pragma clang fp contract(off)
  if (!cfg || sr <= 0 || hop <= 0) return PE_E_ARG;
  for (int i = 0; i < 4; ++i)
    if (!isfinite(cfg[i])) return PE_E_ARG;
  const double flo = cfg[0], cei = cfg[1], ch = cfg[2], ar = cfg[3];
  if (!(flo > 0.0) || !(flo < cei) || !(ch > 0.0) || !(ar > 0.0)) return PE_E_ARG;
  if (sr < 8000 || sr > 48000) return PE_E_UNSUPPORTED;
  if (!(cei < 0.5 * sr) || hop > sr) return PE_E_UNSUPPORTED;
  const double nb = log2(cei / flo) * ch;
  if (nb >= (double)kMaxBands) return PE_E_UNSUPPORTED;
  k->sr = sr;
  k->hop = hop;
  k->frame_period = (double)hop * 1000.0 / (double)sr;
  k->bands = 1 + (int)nb;
  k->cut = (int)round_half_away((double)sr / kLowCut);
  for (int b = 0; b < k->bands; ++b) {
    const double e = (double)(b + 1) / ch;
    k->boundary_d[b] = flo * pow(2.0, e);
    k->boundary[b] = (float)k->boundary_d[b];
    const double h = (double)sr / k->boundary_d[b] / 2.0;
    k->half[b] = (int)round_half_away(h);
    if (k->half[b] < 1) return PE_E_UNSUPPORTED;
  }
  k->taps = 2 * k->cut + 4 * k->half[0];
  long nfft = 1024;
  while (nfft < 2L * k->taps) nfft *= 2;
  if (nfft > 8192) return PE_E_UNSUPPORTED;
  k->nfft = (int)nfft;
  k->log2c = 0;
  while ((2 << k->log2c) < nfft) ++k->log2c;
  k->step = k->nfft - k->taps + 1;
  k->lead = k->cut + 2 * k->half[0] - 1;
  k->vrm = (int)(0.5 + 1000.0 / k->frame_period / flo) * 2 + 1;
  if (!stonemask_fits(sr, flo)) return PE_E_UNSUPPORTED;
  k->floor_d = flo;
  k->floor_f = (float)flo;
  k->ceil_f = (float)cei;
  k->allowed = (float)ar;
  return PE_OK;
}

long table_floats(const DioConsts& k) {       // twiddles (C float2), split roots (C + 1), bands x filter spectrum (C + 1)
  const long C = k.nfft / 2;
  return fft_table_floats(C) + (long)k.bands * 2 * (C + 1);
}

// roots of the 128 .. 4096-point transforms, back to back: the sum of 2 x 2^l floats over l
long stonemask_table_floats() { return (4L << kSmMaxLog2) - (2L << kSmMinLog2); }

long frame_count(long n, const DioConsts& k) {
#pragma clang fp contract(off)
  const double ms = 1000.0 * (double)n / (double)k.sr;
  return (long)(ms / k.frame_period) + 1;
}

constexpr unsigned kCheckBlocks = 1, kCheckFrames = 2;     // `checks`: also hold a row to k's block / frame count

bool meta_ok(const long* hm, int n_rows, unsigned checks, const DioConsts& k, long* totals5) {
  long f = 0, s = 0, b = 0, e = 0, c = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * D_K;
    if ((checks & kCheckBlocks) && m[D_BLOCKS] != (m[D_N] + k.step - 1) / k.step) return false;
    if ((checks & kCheckFrames) && m[D_FRAMES] != frame_count(m[D_N], k)) return false;
    if (m[D_N] < 0 || m[D_N] > (1L << 31) - 8 || m[D_XOFF] < 0 || m[D_FRAMES] < 0 || m[D_BLOCKS] < 0 || m[D_CHUNKS] < 0)
      return false;
    if (m[D_FOFF] != f || m[D_SOFF] != s || m[D_BOFF] != b || m[D_EOFF] != e || m[D_COFF] != c) return false;
    if (m[D_CHUNKS] != (m[D_N] + kChunk - 1) / kChunk) return false;
    f += m[D_FRAMES]; s += m[D_N]; b += m[D_BLOCKS]; e += m[D_N] / 2 + 1; c += m[D_CHUNKS];
  }
  totals5[0] = f; totals5[1] = s; totals5[2] = b; totals5[3] = e; totals5[4] = c;
  return true;
}

// ---- bands -------------------------------------------------------------------------------------------------------------
template <int LOG2C>
__global__ __launch_bounds__(kThreads) void dio_bands_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ tables, int n_rows, long blocks,
                                                             long samples, DioConsts K, float* __restrict__ sig) {
  constexpr int C = 1 << LOG2C, N = 2 * C;
  constexpr int NQ = C / kThreads;
  __shared__ float2 s_buf[C];
  float* fb = reinterpret_cast<float*>(s_buf);
  const float2* tw = reinterpret_cast<const float2*>(tables);
  const float2* tr = tw + C;
  const float2* flt = tr + (C + 1);
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < blocks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, D_K, D_BOFF, g);
    const long* m = meta + (long)row * D_K;
    const long n = m[D_N], o = (g - m[D_BOFF]) * (long)K.step;
    const float* xr = x + m[D_XOFF];
    const float mean = stats[2 * row];
    for (int j = tid; j < N; j += kThreads) {
      const long idx = o + j - K.lead;
      fb[j] = (idx >= 0 && idx < n) ? xr[idx] - mean : 0.f;
    }
    __syncthreads();
    fft_lds<LOG2C, false, kThreads>(s_buf, tw, tid);
    // bins k and C - k of the real transform: X[k] = e + t, conj(X[C - k]) = e - t
    float2 e[NQ], t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = tid + kThreads * q;
      float2 o2;
      t[q] = real_fft_bin(s_buf, tr[k], C, k, e[q], o2);
    }
    __syncthreads();
    for (int b = 0; b < K.bands; ++b) {
      const float2* G = flt + (long)b * (C + 1);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int k = tid + kThreads * q;
        const float2 y1 = cmul(cadd(e[q], t[q]), G[k]);
        const float2 y2 = cmul(csub(e[q], t[q]), conj2(G[C - k]));
        s_buf[k] = real_fft_pack(y1, y2, tr[k]);
      }
      __syncthreads();
      fft_lds<LOG2C, true, kThreads>(s_buf, tw, tid);
      float* out = sig + (long)b * samples + m[D_SOFF] + o;
      for (int r = tid; r < K.step; r += kThreads)
        if (o + r < n) out[r] = fb[r + K.taps - 1];
      __syncthreads();
    }
  }
}

// ---- events ------------------------------------------------------------------------------------------------------------
// Edge of kind 0 / 1 at i: 0 < +-y[i] && +-y[i + 1] <= 0; of kind 2 / 3: the same on d[i] = y[i + 1] - y[i].  Wave w of
// a chunk owns samples [512 w, 512 w + 512) of it, so event order is (wave, pass, lane).
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void dio_events_kernel(const float* __restrict__ sig,
                                                              const long* __restrict__ meta, int n_rows, long chunks,
                                                              long samples, int bands, int* __restrict__ counts,
                                                              const int* __restrict__ base, int* __restrict__ e_idx,
                                                              float* __restrict__ e_frac) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[4][kKinds];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long g = blockIdx.x; g < chunks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, D_K, D_COFF, g);
    const long* m = meta + (long)row * D_K;
    const long n = m[D_N], lo = (g - m[D_COFF]) * (long)kChunk + wave * 512;
    const long cap = n / 2 + 1;
    for (int b = 0; b < bands; ++b) {
      const float* y = sig + (long)b * samples + m[D_SOFF];
      int run[kKinds] = {0, 0, 0, 0};
      // WRITE: a first pass counts this wave's events, the second one starts at the chunk's prefix plus the waves
      // before this one and scatters
      for (int phase = WRITE ? 0 : 1; phase < 2; ++phase) {
        if (WRITE && phase == 1) {
          __syncthreads();                                          // the band before is done with s_cnt
          if (lane == 0)
            for (int k = 0; k < kKinds; ++k) s_cnt[wave][k] = run[k];
          __syncthreads();
          for (int k = 0; k < kKinds; ++k) {
            int st = base[(g * bands + b) * kKinds + k];
            for (int w = 0; w < wave; ++w) st += s_cnt[w][k];
            run[k] = st;
          }
        }
        for (int it = 0; it < 8; ++it) {
          const long i = lo + it * 64 + lane;
          const float x0 = i < n ? y[i] : 0.f, x1 = i + 1 < n ? y[i + 1] : 0.f, x2 = i + 2 < n ? y[i + 2] : 0.f;
          const float d0 = x1 - x0, d1 = x2 - x1;
          const bool p = i + 1 < n, q = i + 2 < n;
          const bool fl[kKinds] = {p && 0.f < x0 && x1 <= 0.f, p && 0.f < -x0 && -x1 <= 0.f,
                                   q && 0.f < d0 && d1 <= 0.f, q && 0.f < -d0 && -d1 <= 0.f};
#pragma unroll
          for (int k = 0; k < kKinds; ++k) {
            const unsigned long long mask = __ballot(fl[k]);
            if (WRITE && phase == 1 && fl[k]) {
              const long at = m[D_EOFF] * (long)bands * kKinds + ((long)b * kKinds + k) * cap + run[k] +
                              __popcll(mask & below);
              const float a = k < 2 ? x0 : d0, c = k < 2 ? x1 : d1;
              e_idx[at] = (int)(i + 1);
              e_frac[at] = a / (a - c);
            }
            run[k] += __popcll(mask);
          }
        }
      }
      if (!WRITE) {
        if (lane == 0)
          for (int k = 0; k < kKinds; ++k) s_cnt[wave][k] = run[k];
        __syncthreads();
        if (tid < kKinds)
          counts[(g * bands + b) * kKinds + tid] = (s_cnt[0][tid] + s_cnt[1][tid]) + (s_cnt[2][tid] + s_cnt[3][tid]);
        __syncthreads();
      }
    }
  }
}

// exclusive prefix of the chunk counts of one (row, band, kind), and its total
__global__ __launch_bounds__(kThreads) void dio_prefix_kernel(const int* __restrict__ counts,
                                                              const long* __restrict__ meta, int n_rows, int bands,
                                                              int* __restrict__ base, int* __restrict__ e_count) {
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int bk = bands * kKinds;
  if (id >= (long)n_rows * bk) return;
  const int row = (int)(id / bk), j = (int)(id % bk);
  const long* m = meta + (long)row * D_K;
  int run = 0;
  for (long c = m[D_COFF]; c < m[D_COFF] + m[D_CHUNKS]; ++c) {
    base[c * bk + j] = run;
    run += counts[c * bk + j];
  }
  e_count[id] = run;
}

// ---- candidates ----------------------------------------------------------------------------------------------------------
// Linear interpolation of one interval track at sample position xs (WORLD's interp1: the end segments extrapolate).
// Interval j lies between fine edges j and j + 1; its location is their mean, its value sr over their difference,
// both from integer differences plus fraction differences.
__device__ __forceinline__ float interval_at(const int* __restrict__ I, const float* __restrict__ F, int edges,
                                             double xs2, float srf) {
#pragma clang fp contract(off)
  const int M = edges - 1;
  int lo = 0, hi = M;                                       // number of intervals whose location <= xs
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double loc2 = (double)(I[mid] + I[mid + 1]) + (double)(F[mid] + F[mid + 1]);
    if (loc2 <= xs2) lo = mid + 1; else hi = mid;
  }
  int k = lo < 1 ? 1 : lo;
  k = k > M - 1 ? M - 1 : k;
  const int a = k - 1;
  const int i0 = I[a], i1 = I[a + 1], i2 = I[a + 2];
  const float f0 = F[a], f1 = F[a + 1], f2 = F[a + 2];
  const float va = srf / ((float)(i1 - i0) + (f1 - f0));
  const float vb = srf / ((float)(i2 - i1) + (f2 - f1));
  const float sa = f0 + f1, sb = f1 + f2;
  const double num = (xs2 - (double)(i0 + i1)) - (double)sa;
  const double den = (double)(i2 - i0) + ((double)sb - (double)sa);
  const float s = (float)num / (float)den;
  return va + s * (vb - va);
}

__global__ __launch_bounds__(kThreads) void dio_candidates_kernel(const int* __restrict__ e_idx,
                                                                  const float* __restrict__ e_frac,
                                                                  const int* __restrict__ e_count,
                                                                  const long* __restrict__ meta, int n_rows, long frames,
                                                                  DioConsts K, float* __restrict__ cand,
                                                                  float* __restrict__ score) {
#pragma clang fp contract(off)
  const long total = frames * K.bands;
  const float srf = (float)K.sr;
  for (long id = (long)blockIdx.x * kThreads + threadIdx.x; id < total; id += (long)gridDim.x * kThreads) {
    const long g = id / K.bands;
    const int b = (int)(id % K.bands);
    const int row = find_row(meta, n_rows, D_K, D_FOFF, g);
    const long* m = meta + (long)row * D_K;
    const long i = g - m[D_FOFF], cap = m[D_N] / 2 + 1;
    const int* ec = e_count + ((long)row * K.bands + b) * kKinds;
    int cnt[kKinds];
    for (int k = 0; k < kKinds; ++k) cnt[k] = ec[k] < cap ? ec[k] : (int)cap;      // never past the row's slots
    float c = 0.f, sc = kRejected;
    // a band is rejected whole unless every kind has at least 3 intervals (4 edges)
    if (cnt[0] >= 4 && cnt[1] >= 4 && cnt[2] >= 4 && cnt[3] >= 4) {
      const double t = (double)i * K.frame_period / 1000.0;
      const double xs2 = 2.0 * (t * (double)K.sr);
      float v[kKinds];
#pragma unroll
      for (int k = 0; k < kKinds; ++k) {
        const long at = m[D_EOFF] * (long)K.bands * kKinds + ((long)b * kKinds + k) * cap;
        v[k] = interval_at(e_idx + at, e_frac + at, cnt[k], xs2, srf);
      }
      const float mean = (((v[0] + v[1]) + v[2]) + v[3]) / 4.f;
      const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
      const float spread = sqrtf((((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) / 3.f);
      const float bd = K.boundary[b];
      const bool out = mean > bd || mean < bd / 2.f || mean > K.ceil_f || mean < K.floor_f;
      if (!out && spread == spread) { c = mean; sc = spread; }
    }
    cand[(long)b * frames + g] = c;
    score[(long)b * frames + g] = sc;
  }
}

__global__ __launch_bounds__(kThreads) void dio_best_kernel(const float* __restrict__ cand,
                                                            const float* __restrict__ score, long frames, int bands,
                                                            float* __restrict__ best, int* __restrict__ best_band) {
  for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < frames; g += (long)gridDim.x * kThreads) {
    float s = score[g], f = cand[g];
    int bb = 0;
    for (int b = 1; b < bands; ++b) {
      const float sb = score[(long)b * frames + g];
      if (s > sb) { s = sb; f = cand[(long)b * frames + g]; bb = b; }
    }
    best[g] = f;
    best_band[g] = bb;
  }
}

// ---- contour fix ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float select_best(float current, float past, const float* __restrict__ cand, long frames,
                                             int bands, long at, float allowed) {
#pragma clang fp contract(off)
  const float ref = (current * 3.f - past) / 2.f;
  float best = cand[at], err = fabsf(ref - best);
  for (int b = 1; b < bands; ++b) {
    const float c = cand[(long)b * frames + at];
    const float e = fabsf(ref - c);
    if (e < err) { err = e; best = c; }
  }
  return fabsf(1.f - best / ref) > allowed ? 0.f : best;
}

// steps[s][g], s = 0 .. 3: the contour after FixStep1 .. FixStep4.  One wave per row; steps 1 and 2 are per-frame
// tests, steps 3 and 4 walk the voiced sections frame by frame (lane 0).
__global__ __launch_bounds__(64) void dio_fix_kernel(const float* __restrict__ best, const float* __restrict__ cand,
                                                     const long* __restrict__ meta, long frames, DioConsts K,
                                                     float* __restrict__ steps) {
#pragma clang fp contract(off)
  const int row = blockIdx.x, lane = threadIdx.x;
  const long* m = meta + (long)row * D_K;
  const long T = m[D_FRAMES], off = m[D_FOFF];
  if (T <= 0) return;
  float* s1 = steps + off;
  float* s2 = s1 + frames;
  float* s3 = s2 + frames;
  float* s4 = s3 + frames;
  const int vrm = K.vrm;
  if (T <= vrm) {
    for (long i = lane; i < T; i += 64) s1[i] = s2[i] = s3[i] = s4[i] = 0.f;
    return;
  }
  const float* bc = best + off;
  auto base = [&](long i) { return (i >= vrm && i < T - vrm) ? bc[i] : 0.f; };
  for (long i = lane; i < T; i += 64) {
    float v = 0.f;
    if (i >= vrm) {
      const float bi = base(i), bp = base(i - 1);
      v = fabsf((bi - bp) / (1e-12f + bi)) < K.allowed ? bi : 0.f;
    }
    s1[i] = v;
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  const int centre = (vrm - 1) / 2;
  for (long i = lane; i < T; i += 64) {
    float v = s1[i];
    if (i >= centre && i < T - centre)
      for (int j = -centre; j <= centre; ++j)
        if (s1[i + j] == 0.f) { v = 0.f; break; }
    s2[i] = v;
    s3[i] = v;
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  if (lane != 0) return;
  const float* cd = cand + off;
  // step 3: from the last frame of every voiced section of s2 forward, up to the next section's last frame
  for (long i = 1; i < T; ++i) {
    if (!(s2[i] == 0.f && s2[i - 1] != 0.f)) continue;
    for (long j = i - 1; j < T - 1; ++j) {
      if (j > i - 1 && s2[j + 1] == 0.f && s2[j] != 0.f) break;
      const float v = select_best(s3[j], s3[j - 1], cd, frames, K.bands, j + 1, K.allowed);
      s3[j + 1] = v;
      if (v == 0.f) break;
    }
  }
  for (long i = 0; i < T; ++i) s4[i] = s3[i];
  // step 4: from the first frame of every section of s2 backward, last section first, down to the one before it
  for (long i = T - 1; i >= 1; --i) {
    if (!(s2[i - 1] == 0.f && s2[i] != 0.f)) continue;
    for (long j = i; j > 1; --j) {
      if (j < i && s2[j - 1] == 0.f && s2[j] != 0.f) break;
      const float v = select_best(s4[j], s4[j + 1], cd, frames, K.bands, j - 1, K.allowed);
      s4[j - 1] = v;
      if (v == 0.f) break;
    }
  }
}

// ---- StoneMask -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fix_f0(const float2* __restrict__ z, int N, float srf, float f, int harmonics,
                                        float unscale) {
#pragma clang fp contract(off)
  float num = 0.f, den = 0.f;
  for (int h = 0; h < harmonics; ++h) {
    const int idx = (int)floor((double)f * (double)N / (double)srf * (double)(h + 1) + 0.5);
    const float2 zk = z[idx & (N - 1)], zc = conj2(z[(N - idx) & (N - 1)]);
    const float mr = 0.5f * (zk.x + zc.x), mi = 0.5f * (zk.y + zc.y);          // main spectrum
    const float dr = 0.5f * (zk.y - zc.y), di = -0.5f * (zk.x - zc.x);         // difference spectrum
    const float nm = (mr * di - mi * dr) * unscale, pw = mr * mr + mi * mi;
    const float inst = pw == 0.f ? 0.f : (float)idx * srf / (float)N + nm / pw * srf / 2.f / kPiF;
    const float amp = sqrtf(pw);
    num = num + amp * inst;
    den = den + amp * (float)(h + 1);
  }
  return num / den;
}

__global__ __launch_bounds__(kThreads) void stonemask_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                             const float* __restrict__ f0_in,
                                                             const float* __restrict__ roots, int n_rows, long frames,
                                                             int sr, double frame_period, float f0_min,
                                                             float* __restrict__ f0_out) {
  constexpr int CMAX = 1 << kSmMaxLog2;
  __shared__ float2 s_buf[CMAX];
  __shared__ float s_w[CMAX + 2];
  const int tid = threadIdx.x;
  const float srf = (float)sr;
  for (long g = blockIdx.x; g < frames; g += gridDim.x) {
    const float f0 = f0_in[g];
    if (!(f0 > 0.f)) {                                              // uniform over the workgroup
      if (tid == 0) f0_out[g] = 0.f;
      continue;
    }
    if (f0 <= 40.f || f0 > srf / 12.f || f0 < f0_min) {
      if (tid == 0) f0_out[g] = 0.f;
      continue;
    }
    const int row = find_row(meta, n_rows, D_K, D_FOFF, g);
    const long* m = meta + (long)row * D_K;
    const long n = m[D_N];
    const float* xr = x + m[D_XOFF];
    int half, len, lg;
    double t;
    {
#pragma clang fp contract(off)
      half = (int)(1.5 * (double)sr / (double)f0 + 1.0);
      len = 2 * half + 1;
      lg = 2 + (31 - __builtin_clz(len));
      t = (double)(g - m[D_FOFF]) * frame_period / 1000.0;
    }
    if (lg > kSmMaxLog2 || n <= 0) {                                // below f0_min by the plan's check; kept for safety
      if (tid == 0) f0_out[g] = 0.f;
      continue;
    }
    const int N = 1 << lg;
    // The difference window is about 2 pi f0 / sr = 9.4 / half times the main one at the first harmonic, and the
    // rounding of the shared transform is relative to the larger of its two inputs: the imaginary input is scaled up
    // by a power of two (N / 128, about half / 8 .. half / 16) and the numerator scaled back, both exactly.
    const float scale = (float)(1 << (lg - kSmMinLog2)), unscale = 1.f / scale;
    for (int j = tid; j < len + 2; j += kThreads) {
      float w = 0.f;
      if (j >= 1 && j <= len) {
#pragma clang fp contract(off)
        const double pos = (t + (double)(j - 1 - half) / (double)sr) * (double)sr;
        const double raw = pos < 0.0 ? -floor(-pos + 0.5) : floor(pos + 0.5);
        const double tmp = (raw - 1.0) / (double)sr - t;
        const float u = (float)(tmp / ((double)len / (double)sr));
        w = 0.42f + 0.5f * cospif(2.f * u) + 0.08f * cospif(4.f * u);
      }
      s_w[j] = w;
    }
    __syncthreads();
    for (int j = tid; j < N; j += kThreads) {
      float2 v = make_float2(0.f, 0.f);
      if (j < len) {
#pragma clang fp contract(off)
        const double pos = (t + (double)(j - half) / (double)sr) * (double)sr;
        const double raw = pos < 0.0 ? -floor(-pos + 0.5) : floor(pos + 0.5);
        long idx = (long)raw - 1;
        idx = idx < 0 ? 0 : (idx > n - 1 ? n - 1 : idx);
        const float s = xr[idx];
        v = make_float2(s * s_w[j + 1], s * (-(s_w[j + 2] - s_w[j]) / 2.f) * scale);
      }
      s_buf[j] = v;
    }
    __syncthreads();
    long ro = 0;
    for (int l = kSmMinLog2; l < lg; ++l) ro += 1L << l;
    const float2* tw = reinterpret_cast<const float2*>(roots) + ro;
    switch (lg) {                                                   // uniform over the workgroup (host: with_log2)
      case 7: fft_lds<7, false, kThreads>(s_buf, tw, tid); break;
      case 8: fft_lds<8, false, kThreads>(s_buf, tw, tid); break;
      case 9: fft_lds<9, false, kThreads>(s_buf, tw, tid); break;
      case 10: fft_lds<10, false, kThreads>(s_buf, tw, tid); break;
      case 11: fft_lds<11, false, kThreads>(s_buf, tw, tid); break;
      default: fft_lds<12, false, kThreads>(s_buf, tw, tid); break;
    }
    if (tid == 0) {
#pragma clang fp contract(off)
      float r = 0.f;
      const float first = fix_f0(s_buf, N, srf, f0, 2, unscale);
      if (!(first <= 0.f) && !(first > f0 * 2.f) && first == first) {
        int nh = (int)((double)srf / 2.0 / (double)first);
        nh = nh < 6 ? nh : 6;
        r = fix_f0(s_buf, N, srf, first, nh, unscale);
      }
      if (!(fabsf(r - f0) <= f0 * 0.2f)) r = f0;
      f0_out[g] = r;
    }
    __syncthreads();
  }
}

// ---- what every stage entry point checks before its own pointers: host_meta is the plan's; `work`: the total a launch
// needs (-1: none) ----------------------------------------------------------------------------------------------------------
struct DioBatch { DioConsts k; long tot[5]; };        // tot: the batch's totals by meta_ok, indexed by TOT_*
enum { TOT_FRAMES, TOT_SAMPLES, TOT_BLOCKS, TOT_SLOTS, TOT_CHUNKS };

// `config`: derive's status for b->k (PE_OK where an entry point has no config and `checks` none of b->k)
int open_batch(int n_rows, int config, const long* host_meta, unsigned checks, int work, DioBatch* b) {
  return open_rows(n_rows, config, host_meta, [&] { return meta_ok(host_meta, n_rows, checks, b->k, b->tot); },
                   work >= 0 ? &b->tot[work] : nullptr);
}

int open_batch(int n_rows, int sr, int hop, const double* config4, const long* host_meta, unsigned checks, int work,
               DioBatch* b) {
  return open_batch(n_rows, derive(sr, hop, config4, &b->k), host_meta, checks, work, b);
}

}  // namespace

extern "C" int pe_f0_dio_plan_fields(void) { return D_K; }

/* Host-only layout; see include/pitchextractor_hip.h. */
extern "C" int pe_f0_dio_plan(int n_rows, const long* n, const long* x_off, int sr, int hop, const double* config4,
                              long* consts10, long* half16, double* dconsts17, long* meta, long* totals6) {
  DioConsts k;
  if (!config4 || !consts10 || !half16 || !dconsts17 || !totals6 || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows > 0 && (!n || !x_off || !meta)) return PE_E_ARG;
  const int st = derive(sr, hop, config4, &k);
  if (st != PE_OK) return st;
  for (int r = 0; r < n_rows; ++r)
    if (n[r] < 0 || n[r] > (1L << 31) - 8 || x_off[r] < 0) return PE_E_ARG;
  consts10[0] = k.bands; consts10[1] = k.nfft; consts10[2] = k.taps; consts10[3] = k.step; consts10[4] = k.lead;
  consts10[5] = k.vrm; consts10[6] = table_floats(k); consts10[7] = kChunk; consts10[8] = k.cut;
  consts10[9] = stonemask_table_floats();
  dconsts17[0] = k.frame_period;
  for (int b = 0; b < kMaxBands; ++b) {
    half16[b] = b < k.bands ? k.half[b] : 0;
    dconsts17[1 + b] = b < k.bands ? k.boundary_d[b] : 0.0;
  }
  long f = 0, s = 0, bl = 0, e = 0, c = 0;
  for (int r = 0; r < n_rows; ++r) {
    long* m = meta + (long)r * D_K;
    m[D_XOFF] = x_off[r]; m[D_N] = n[r];
    m[D_FRAMES] = frame_count(n[r], k); m[D_FOFF] = f;
    m[D_SOFF] = s;
    m[D_BLOCKS] = (n[r] + k.step - 1) / k.step; m[D_BOFF] = bl;
    m[D_EOFF] = e;
    m[D_CHUNKS] = (n[r] + kChunk - 1) / kChunk; m[D_COFF] = c;
    f += m[D_FRAMES]; s += n[r]; bl += m[D_BLOCKS]; e += n[r] / 2 + 1; c += m[D_CHUNKS];
  }
  totals6[0] = f; totals6[1] = s; totals6[2] = bl; totals6[3] = e; totals6[4] = c;
  totals6[5] = 2 * c * k.bands * kKinds * (long)sizeof(int);        // workspace of pe_f0_dio_events
  return PE_OK;
}

extern "C" int pe_f0_dio_bands(const float* x, const long* meta, const long* host_meta, const float* stats,
                               const float* tables, long n_table, int n_rows, int sr, int hop, const double* config4,
                               float* band_signals, void* stream) {
  DioBatch b;
  PE_OPEN(open_batch(n_rows, sr, hop, config4, host_meta, kCheckBlocks, TOT_BLOCKS, &b));
  if (!x || !meta || !stats || !tables || !band_signals) return PE_E_ARG;
  if (n_table != table_floats(b.k)) return PE_E_ARG;
  return with_log2<9, 12>(b.k.log2c, [&](auto L) {
    hipLaunchKernelGGL(dio_bands_kernel<decltype(L)::value>, dim3(grid_of(b.tot[TOT_BLOCKS])), dim3(kThreads), 0,
                       pe_stream(stream), x, meta, stats, tables, n_rows, b.tot[TOT_BLOCKS], b.tot[TOT_SAMPLES], b.k,
                       band_signals);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

extern "C" int pe_f0_dio_events(const float* band_signals, const long* meta, const long* host_meta, int n_rows, int sr,
                                int hop, const double* config4, int* e_idx, float* e_frac, int* e_count,
                                void* workspace, size_t workspace_bytes, void* stream) {
  DioBatch b;
  PE_OPEN(open_batch(n_rows, sr, hop, config4, host_meta, 0, -1, &b));
  if (!meta || !e_count) return PE_E_ARG;
  const long chunks = b.tot[TOT_CHUNKS], samples = b.tot[TOT_SAMPLES];
  const int bands = b.k.bands;
  const size_t half_ws = (size_t)chunks * bands * kKinds * sizeof(int);
  if (chunks > 0) {
    if (!band_signals || !e_idx || !e_frac) return PE_E_ARG;
    if (!workspace || workspace_bytes < 2 * half_ws) return PE_E_WORKSPACE;
  }
  int* counts = static_cast<int*>(workspace);
  int* base = counts + (size_t)chunks * bands * kKinds;
  if (chunks > 0) {
    hipLaunchKernelGGL(dio_events_kernel<false>, dim3(grid_of(chunks)), dim3(kThreads), 0, pe_stream(stream),
                       band_signals, meta, n_rows, chunks, samples, bands, counts, base, e_idx, e_frac);
    PE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dio_prefix_kernel, dim3(pe_cdiv((long)n_rows * bands * kKinds, kThreads)), dim3(kThreads), 0,
                     pe_stream(stream), counts, meta, n_rows, bands, base, e_count);
  PE_LAUNCH_CHECK();
  if (chunks > 0) {
    hipLaunchKernelGGL(dio_events_kernel<true>, dim3(grid_of(chunks)), dim3(kThreads), 0, pe_stream(stream),
                       band_signals, meta, n_rows, chunks, samples, bands, counts, base, e_idx, e_frac);
    PE_LAUNCH_CHECK();
  }
  return PE_OK;
}

extern "C" int pe_f0_dio_candidates(const int* e_idx, const float* e_frac, const int* e_count, const long* meta,
                                    const long* host_meta, int n_rows, int sr, int hop, const double* config4,
                                    float* cand, float* score, float* best, int* best_band, void* stream) {
  DioBatch b;
  PE_OPEN(open_batch(n_rows, sr, hop, config4, host_meta, kCheckFrames, TOT_FRAMES, &b));
  if (!e_idx || !e_frac || !e_count || !meta || !cand || !score || !best || !best_band) return PE_E_ARG;
  const long frames = b.tot[TOT_FRAMES];
  hipLaunchKernelGGL(dio_candidates_kernel, dim3(grid_of(pe_cdiv(frames * b.k.bands, kThreads))), dim3(kThreads), 0,
                     pe_stream(stream), e_idx, e_frac, e_count, meta, n_rows, frames, b.k, cand, score);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(dio_best_kernel, dim3(grid_of(pe_cdiv(frames, kThreads))), dim3(kThreads), 0, pe_stream(stream),
                     cand, score, frames, b.k.bands, best, best_band);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_f0_dio_fix(const float* best, const float* cand, const long* meta, const long* host_meta, int n_rows,
                             int sr, int hop, const double* config4, float* steps4, void* stream) {
  DioBatch b;
  PE_OPEN(open_batch(n_rows, sr, hop, config4, host_meta, 0, TOT_FRAMES, &b));
  if (!best || !cand || !meta || !steps4) return PE_E_ARG;
  hipLaunchKernelGGL(dio_fix_kernel, dim3(n_rows), dim3(64), 0, pe_stream(stream), best, cand, meta, b.tot[TOT_FRAMES],
                     b.k, steps4);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_f0_stonemask(const float* x, const long* meta, const long* host_meta, const float* f0_in,
                               const float* roots, long n_roots, int n_rows, int sr, int hop, double f0_min,
                               float* f0_out, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || sr <= 0 || hop <= 0 || !isfinite(f0_min) || !(f0_min > 0.0)) return PE_E_ARG;
  if (sr < 8000 || sr > 48000 || hop > sr || !stonemask_fits(sr, f0_min)) return PE_E_UNSUPPORTED;
  DioBatch b;
  PE_OPEN(open_batch(n_rows, PE_OK, host_meta, 0, TOT_FRAMES, &b));
  if (!x || !meta || !f0_in || !roots || !f0_out) return PE_E_ARG;
  if (n_roots != stonemask_table_floats()) return PE_E_ARG;
  const double frame_period = (double)hop * 1000.0 / (double)sr;
  hipLaunchKernelGGL(stonemask_kernel, dim3(grid_of(b.tot[TOT_FRAMES])), dim3(kThreads), 0, pe_stream(stream), x, meta,
                     f0_in, roots, n_rows, b.tot[TOT_FRAMES], sr, frame_period, (float)f0_min, f0_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
