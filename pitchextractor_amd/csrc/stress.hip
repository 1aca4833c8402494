// Robustness stress conditions of the reference's evaluation notebooks (Utils/room_and_microphone_stress.ipynb,
// Utils/amplitude_pathologies.ipynb) and their melody metrics (compute_metrics), on ragged batches.  Pinned by the
// float64 restatement in tests/stress_ref.py.
//
// pe_stress_plan (host only) lays the rows out: offset and length (the shared row header), the row's offset in the
// output, its sample prefix and its blocks of kStep samples with their prefix.  Every condition is a fixed number of
// launches whatever the rows are:
//   rir:      spectra (one workgroup per block: the packed real transform of 2 kStep samples, fft_lds), convolve (one
//             workgroup per (row, output block): sum over the RIR's partitions in registers, one inverse transform,
//             kStep samples and their max |y|), normalize (row peak = max of its block peaks, then the scale).  The
//             RIR set is a ragged batch of its own whose blocks are the partitions; its spectra are made by the same
//             kernel and kept by the caller.
//   biquad:   one wave per row, lane s runs stage s one sample behind lane s - 1 (the clamp between two stages makes a
//             stage's input the stored float32 of the one before); state and sums in double.
//   clip:     one workgroup per row: radix select of the two order statistics on the bit pattern of |x| (LDS
//             histograms, integer atomics), numpy's interpolation, the clip.
//   agc:      walk (one wave per row: the envelope follower in double by one lane, the gains by all), then smooth and
//             apply (window sums of float32 gains in double are exact, so their order is free).
//   metrics:  one workgroup per row, integer counts.
// No float atomics, no cross-workgroup communication inside a launch, and nothing a row computes depends on where the
// row lies: a row's result is the same alone, packed or padded.
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;
constexpr int kLog2C = 11, kC = 1 << kLog2C;     // packed transform of 2 kC = 4096 real samples, 16 KB of LDS
constexpr int kStep = kC;                        // block step S = 2048: half of a transform is new
constexpr int kNQ = kC / kThreads;
constexpr int kMaxStages = 8;
constexpr int kPiece = 512;                      // samples a wave stages in LDS per pass (biquad, agc walk)
constexpr int kClipChunk = 4 * kThreads;         // samples per histogram pass of a workgroup
constexpr int kRun = 8;                          // consecutive outputs of one thread of the smoothing kernel
constexpr long kMaxSamples = (1L << 31) - 8;

enum { S_XOFF, S_N, S_YOFF, S_SOFF, S_BLOCKS, S_BOFF, S_K };
static_assert(S_XOFF == kRowOffset && S_N == kRowLength, "the plan opens with the shared row header");
enum { TOT_SAMPLES, TOT_BLOCKS };

constexpr long kTableFloats = fft_table_floats(kC);           // roots of the packed transform, split roots

bool meta_ok(const long* hm, int n_rows, long* totals2) {
  long s = 0, b = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * S_K;
    if (m[S_N] < 0 || m[S_N] > kMaxSamples || m[S_XOFF] < 0 || m[S_YOFF] < 0) return false;
    if (m[S_BLOCKS] != (m[S_N] + kStep - 1) / kStep || m[S_SOFF] != s || m[S_BOFF] != b) return false;
    s += m[S_N]; b += m[S_BLOCKS];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_BLOCKS] = b;
  return true;
}

int open_batch(int n_rows, const long* host_meta, long* totals2) {
  return open_rows(n_rows, PE_OK, host_meta, [&] { return meta_ok(host_meta, n_rows, totals2); },
                   &totals2[TOT_SAMPLES]);
}

// ---- rir -----------------------------------------------------------------------------------------------------------
// Block b of a row as a packed spectrum: bins 1 .. C - 1 of the 2C-point real transform, and {X[0], X[C]} (both real)
// in slot 0.  partition == 0: samples [(b - 1) S, (b + 1) S) of the row, zero outside it (an input block of overlap-
// save); partition == 1: samples [b S, (b + 1) S) followed by S zeros, divided by C (a partition of a filter: the
// inverse transform is not normalised).
__global__ __launch_bounds__(kThreads) void stress_spectra_kernel(const float* __restrict__ x,
                                                                  const long* __restrict__ meta,
                                                                  const float* __restrict__ tables, int n_rows,
                                                                  long blocks, int partition,
                                                                  float2* __restrict__ spectra) {
  __shared__ float2 s_buf[kC];
  float* fb = reinterpret_cast<float*>(s_buf);
  const float2* tw = reinterpret_cast<const float2*>(tables);
  const float2* tr = tw + kC;
  const int tid = threadIdx.x;
  const float scale = partition ? 1.f / kC : 1.f;
  const int span = partition ? kStep : 2 * kStep;
  for (long g = blockIdx.x; g < blocks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_BOFF, g);
    const long* m = meta + (long)row * S_K;
    const long n = m[S_N], b = g - m[S_BOFF];
    const long first = partition ? b * kStep : (b - 1) * kStep;
    const float* xr = x + m[S_XOFF];
    for (int j = tid; j < 2 * kC; j += kThreads) {
      const long idx = first + j;
      fb[j] = (j < span && idx >= 0 && idx < n) ? xr[idx] * scale : 0.f;
    }
    __syncthreads();
    fft_lds<kLog2C, false, kThreads>(s_buf, tw, tid);
    float2* out = spectra + g * kC;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      const int k = tid + kThreads * q;
      float2 e, o;
      const float2 t = real_fft_bin(s_buf, tr[k], kC, k, e, o);
      const float2 v = cadd(e, t);
      out[k] = k == 0 ? make_float2(e.x + o.x, e.x - o.x) : v;
    }
    __syncthreads();
  }
}

// Output block b of a row: Y = sum over p <= min(b, P - 1) of X[b - p] H[p], inverted once; the second half of the
// transform is the block (overlap-save).
__global__ __launch_bounds__(kThreads) void stress_rir_convolve_kernel(const float2* __restrict__ xs,
                                                                       const long* __restrict__ meta,
                                                                       const float2* __restrict__ hs,
                                                                       const long* __restrict__ rir_meta,
                                                                       const int* __restrict__ rir_index,
                                                                       const float* __restrict__ tables, int n_rows,
                                                                       long blocks, float* __restrict__ y,
                                                                       float* __restrict__ peak) {
  __shared__ float2 s_buf[kC];
  __shared__ float s_red[kThreads / 64];
  float* fb = reinterpret_cast<float*>(s_buf);
  const float2* tw = reinterpret_cast<const float2*>(tables);
  const float2* tr = tw + kC;
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < blocks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_BOFF, g);
    const long* m = meta + (long)row * S_K;
    const long n = m[S_N], b = g - m[S_BOFF];
    const long* rm = rir_meta + (long)rir_index[row] * S_K;
    const long parts = rm[S_BLOCKS] < b + 1 ? rm[S_BLOCKS] : b + 1;
    const float2* X = xs + g * kC;
    const float2* H = hs + rm[S_BOFF] * kC;
    float2 acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) acc[q] = make_float2(0.f, 0.f);
    for (long p = 0; p < parts; ++p) {
      const float2* Xp = X - p * kC;
      const float2* Hp = H + p * kC;
      float2 xv[kNQ], hv[kNQ];
#pragma unroll
      for (int q = 0; q < kNQ; ++q) { xv[q] = Xp[tid + kThreads * q]; hv[q] = Hp[tid + kThreads * q]; }
#pragma unroll
      for (int q = 0; q < kNQ; ++q) {
        float2 pr = cmul(xv[q], hv[q]);
        if (tid + kThreads * q == 0) pr = make_float2(xv[q].x * hv[q].x, xv[q].y * hv[q].y);      // X[0] H[0], X[C] H[C]
        acc[q] = cadd(acc[q], pr);
      }
    }
#pragma unroll
    for (int q = 0; q < kNQ; ++q) s_buf[tid + kThreads * q] = acc[q];
    __syncthreads();
    // back to the packed transform's bins: z[k] = ye + i yo, from Y[k] and conj(Y[C - k])
    float2 z[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      const int k = tid + kThreads * q;
      const float2 y1 = k == 0 ? make_float2(s_buf[0].x, 0.f) : s_buf[k];
      const float2 y2 = k == 0 ? make_float2(s_buf[0].y, 0.f) : conj2(s_buf[kC - k]);
      z[q] = real_fft_pack(y1, y2, tr[k]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kNQ; ++q) s_buf[tid + kThreads * q] = z[q];
    __syncthreads();
    fft_lds<kLog2C, true, kThreads>(s_buf, tw, tid);
    float* out = y + m[S_YOFF] + b * kStep;
    float pk = 0.f;
    for (int r = tid; r < kStep; r += kThreads)
      if (b * kStep + r < n) {
        const float v = fb[kStep + r];
        out[r] = v;
        pk = fmaxf(pk, fabsf(v));
      }
    pk = block_max(pk, s_red, tid);             // its barrier: every read of fb is done before the next block's writes
    if (tid == 0) peak[g] = pk;
  }
}

// p = max |y| of the row (the max of its block peaks, whatever the order); p > 0.99: y /= p + 1e-6, in float32: not
// the rounding of float32(double(p) + 1e-6) in the mix of snr_mix.h, so the two stay apart
__global__ __launch_bounds__(kThreads) void stress_rir_normalize_kernel(const long* __restrict__ meta,
                                                                        const float* __restrict__ peak, int n_rows,
                                                                        long blocks, float* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ float s_red[kThreads / 64];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < blocks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_BOFF, g);
    const long* m = meta + (long)row * S_K;
    const long n = m[S_N], b = g - m[S_BOFF];
    float pk = 0.f;
    for (long i = tid; i < m[S_BLOCKS]; i += kThreads) pk = fmaxf(pk, peak[m[S_BOFF] + i]);
    const float p = block_max(pk, s_red, tid);
    if (p > 0.99f) {
      const float d = p + 1e-6f;
      float* out = y + m[S_YOFF] + b * kStep;
      for (int r = tid; r < kStep; r += kThreads)
        if (b * kStep + r < n) out[r] = out[r] / d;
    }
  }
}

// ---- biquad cascade ------------------------------------------------------------------------------------------------
struct Biquads { int stages; double c[kMaxStages][5]; };        // per stage {b0, b1, b2, a1, a2}, a0 = 1

// the value of the lane below (lanes 0, 16, 32, 48: 0)
__device__ __forceinline__ float lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));        // row_shr:1
}

// Lane s < stages holds stage s: its last two inputs and its last two (unclamped) outputs in double.  At step u of a
// piece lane s takes sample u - s: lane 0 from the piece, lane s from what lane s - 1 stored one step before (float32,
// clamped to [-1, 1]: the storage between two stages).  The last stage's stores are the piece of the output.
__global__ __launch_bounds__(64) void stress_biquad_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                           Biquads K, float* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ float s_x[kPiece], s_y[kPiece];
  const int lane = threadIdx.x;
  const long* m = meta + (long)blockIdx.x * S_K;
  const long n = m[S_N];
  const float* xr = x + m[S_XOFF];
  float* yr = y + m[S_YOFF];
  const int st = lane < K.stages ? lane : 0;
  const double b0 = K.c[st][0], b1 = K.c[st][1], b2 = K.c[st][2], a1 = K.c[st][3], a2 = K.c[st][4];
  const bool last = lane == K.stages - 1;
  double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
  float stored = 0.f;
  for (long c0 = 0; c0 < n; c0 += kPiece) {
    const int len = (int)(n - c0 < kPiece ? n - c0 : kPiece);
    for (int j = lane; j < len; j += 64) s_x[j] = xr[c0 + j];
    wave_lds_sync();
    float xv = 0.f;
    for (int u = 0; u < len + K.stages - 1; ++u) {
      if ((u & 63) == 0) xv = u + lane < len ? s_x[u + lane] : 0.f;
      const float head = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv), u & 63));
      const float below = lane_below(stored);
      const int i = u - lane;
      if (lane < K.stages && i >= 0 && i < len) {
        const double in = (double)(lane == 0 ? head : below);
        const double v = b0 * in + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
        x2 = x1; x1 = in; y2 = y1; y1 = v;
        stored = fminf(fmaxf((float)v, -1.f), 1.f);
        if (last) s_y[i] = stored;
      }
    }
    wave_lds_sync();
    for (int j = lane; j < len; j += 64) yr[c0 + j] = s_y[j];
    wave_lds_sync();
  }
}

// ---- clip ----------------------------------------------------------------------------------------------------------
// copy != 0: y = x.  Else thr = numpy's linear quantile of |x| at q, in the arithmetic numpy 2 uses for a float32
// array and a Python float q: everything in float32 (q itself, the virtual index (n - 1) q, the weight, the
// interpolation).  thr <= 0: y = x, else y = clip(x, -thr, thr).  thr_out[row] = thr (NaN for a copy).  q_rows and
// copy_rows (pe_stress_clip_rows; null: q and copy serve every row) hold one q and one copy per row.
__global__ __launch_bounds__(kThreads) void stress_clip_kernel(const float* __restrict__ x,
                                                               const long* __restrict__ meta, float q, int copy,
                                                               const double* __restrict__ q_rows,
                                                               const int* __restrict__ copy_rows,
                                                               float* __restrict__ y, float* __restrict__ thr_out) {
#pragma clang fp contract(off)
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[3];             // digit, rank inside the digit, count of the digit
  __shared__ unsigned s_min;
  const int tid = threadIdx.x;
  if (q_rows) { q = (float)q_rows[blockIdx.x]; copy = copy_rows[blockIdx.x]; }
  const long* m = meta + (long)blockIdx.x * S_K;
  const long n = m[S_N];
  const float* xr = x + m[S_XOFF];
  float* yr = y + m[S_YOFF];
  float thr = __int_as_float(0x7fc00000);
  if (!copy && n > 0) {
    const float v = (float)(n - 1) * q;
    const float fl = floorf(v), gam = v - fl;
    const long k0 = (long)fl < n - 1 ? (long)fl : n - 1;
    const long k1 = k0 + 1 < n - 1 ? k0 + 1 : n - 1;
    unsigned prefix = 0, rank = (unsigned)k0, count = 0;
    for (int pass = 3; pass >= 0; --pass) {
      const int shift = 8 * pass;
      const unsigned mask = pass == 3 ? 0u : 0xffffffffu << (shift + 8);
      s_hist[tid] = 0;
      __syncthreads();
      for (long c0 = 0; c0 < n; c0 += kClipChunk)
        for (int j = tid; j < kClipChunk; j += kThreads)
          if (c0 + j < n) {
            const unsigned key = __float_as_uint(xr[c0 + j]) & 0x7fffffffu;
            if ((key & mask) == (prefix & mask)) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
          }
      __syncthreads();
      if (tid == 0) {
        unsigned cum = 0, d = 0;
        for (; d < 255; ++d) {
          if (rank < cum + s_hist[d]) break;
          cum += s_hist[d];
        }
        s_sel[0] = d; s_sel[1] = rank - cum; s_sel[2] = s_hist[d];
      }
      __syncthreads();
      prefix |= s_sel[0] << shift;
      rank = s_sel[1];
      count = s_sel[2];
      __syncthreads();
    }
    // s[k0] = prefix, at position `rank` among its `count` copies; s[k1] is another copy or the next key above
    unsigned next = prefix;
    if ((unsigned)(k1 - k0) + rank >= count) {
      if (tid == 0) s_min = 0xffffffffu;
      __syncthreads();
      unsigned lo = 0xffffffffu;
      for (long c0 = 0; c0 < n; c0 += kClipChunk)
        for (int j = tid; j < kClipChunk; j += kThreads)
          if (c0 + j < n) {
            const unsigned key = __float_as_uint(xr[c0 + j]) & 0x7fffffffu;
            if (key > prefix && key < lo) lo = key;
          }
      atomicMin(&s_min, lo);
      __syncthreads();
      next = s_min;
    }
    const float lo_v = __uint_as_float(prefix), hi_v = __uint_as_float(next);
    const float d = hi_v - lo_v;
    thr = gam >= 0.5f ? hi_v - d * (1.f - gam) : lo_v + d * gam;
  }
  const bool clip = !copy && thr > 0.f;
  for (long i = tid; i < n; i += kThreads) {
    const float v = xr[i];
    yr[i] = clip ? fminf(fmaxf(v, -thr), thr) : v;
  }
  if (thr_out && tid == 0) thr_out[blockIdx.x] = thr;
}

// ---- agc -----------------------------------------------------------------------------------------------------------
struct AgcParams { double attack, release, target, max_gain; int smoothing; };

// env follows |x| with the attack coefficient upwards and the release coefficient downwards, as the reference's Python
// floats do (two products and a sum, never fused); gain = float32(clip(target / (env + 1e-6), 1 / max_gain, max_gain)).
__global__ __launch_bounds__(64) void stress_agc_walk_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                             AgcParams P, float* __restrict__ gains) {
#pragma clang fp contract(off)
  __shared__ float s_x[kPiece];
  __shared__ double s_env[kPiece];
  const int lane = threadIdx.x;
  const long* m = meta + (long)blockIdx.x * S_K;
  const long n = m[S_N];
  const float* xr = x + m[S_XOFF];
  float* gr = gains + m[S_SOFF];
  const double a = P.attack, oma = 1.0 - P.attack, rl = P.release, omr = 1.0 - P.release;
  const double g_lo = 1.0 / P.max_gain, g_hi = P.max_gain;
  double env = 0.0;
  for (long c0 = 0; c0 < n; c0 += kPiece) {
    const int len = (int)(n - c0 < kPiece ? n - c0 : kPiece);
    for (int j = lane; j < len; j += 64) s_x[j] = xr[c0 + j];
    wave_lds_sync();
    if (lane == 0) {
      for (int j0 = 0; j0 < len; j0 += 8) {
        double r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = fabs((double)s_x[j0 + u < len ? j0 + u : len - 1]);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (j0 + u < len) {
            env = r[u] > env ? a * env + oma * r[u] : rl * env + omr * r[u];
            s_env[j0 + u] = env;
          }
      }
    }
    wave_lds_sync();
    for (int j = lane; j < len; j += 64) {
      const double desired = P.target / (s_env[j] + 1e-6);
      gr[c0 + j] = (float)fmin(fmax(desired, g_lo), g_hi);
    }
    wave_lds_sync();
  }
}

// np.convolve(gains, ones(s) / s, "same"): out[i] = (1 / s) sum over m < s of g[i + (s - 1) / 2 - m], zero outside the
// row.  Gains are float32 in [1 / max_gain, max_gain] with max_gain < 2^8, so every sum or difference of sums of up to
// 2^13 of them is exact in double and the order is free.  A workgroup takes kStep outputs: it sums the first window
// together, thread t adds what enters and leaves the window over the kRun outputs before its own, a scan of those
// differences gives every thread its first window, and the thread slides it over its kRun outputs.  Rounded once to
// float32; then y = clip(float32(x g), -1, 1).
__global__ __launch_bounds__(kThreads) void stress_agc_apply_kernel(const float* __restrict__ x,
                                                                    const long* __restrict__ meta,
                                                                    const float* __restrict__ gains, int n_rows,
                                                                    long blocks, int s, float* __restrict__ y) {
#pragma clang fp contract(off)
  static_assert(kRun * kThreads == kStep, "one thread per run of a block");
  __shared__ double s_sum[kThreads];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < blocks; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_BOFF, g);
    const long* m = meta + (long)row * S_K;
    const long n = m[S_N], base = (g - m[S_BOFF]) * kStep, i0 = base + (long)tid * kRun;
    const float* xr = x + m[S_XOFF];
    const float* gr = gains + m[S_SOFF];
    float* yr = y + m[S_YOFF];
    const long h = (s - 1) / 2;
    auto at = [&](long j) { return j >= 0 && j < n ? (double)gr[j] : 0.0; };
    double sum = 0.0;
    if (s > 1) {
      // the window of output `base`
      double part = 0.0;
      for (long j = base + h - s + 1 + tid; j <= base + h; j += kThreads) part += at(j);
      s_sum[tid] = part;
      __syncthreads();
      for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (tid < st) s_sum[tid] += s_sum[tid + st];
        __syncthreads();
      }
      const double first = s_sum[0];
      __syncthreads();
      // window(i0) - window(i0 - kRun), then its inclusive scan over the threads
      double delta = 0.0;
      if (tid > 0)
        for (int u = 1; u <= kRun; ++u) delta += at(i0 - kRun + h + u) - at(i0 - kRun + h + u - s);
      s_sum[tid] = delta;
      __syncthreads();
      for (int st = 1; st < kThreads; st <<= 1) {
        const double add = tid >= st ? s_sum[tid - st] : 0.0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
      }
      sum = first + s_sum[tid];
      __syncthreads();
    }
    for (int u = 0; u < kRun && i0 + u < n; ++u) {
      const long i = i0 + u;
      if (s > 1 && u > 0) sum += at(i + h) - at(i + h - s);
      const float gain = s > 1 ? (float)(sum / (double)s) : gr[i];
      const float v = xr[i] * gain;
      yr[i] = fminf(fmaxf(v, -1.f), 1.f);
    }
  }
}

// ---- melody metrics ------------------------------------------------------------------------------------------------
enum { M_POFF, M_N, M_ROFF, M_BOFF, M_NFLIP, M_K };           // tracks: pred offset, frames, ref offset, baseline offset
static_assert(M_POFF == kRowOffset && M_N == kRowLength, "the track plan opens with the shared row header");
constexpr int kCounts = 6;

// The notebooks' compute_metrics over the row's first M_N frames, in double; VUV_flips over the first M_NFLIP frames of
// the prediction and the baseline.  out7 = {RPA, RCA, VUV accuracy, OctaveError, VUV_flips, voiced frames, frames}.
__global__ __launch_bounds__(kThreads) void stress_melody_metrics_kernel(const float* __restrict__ pred,
                                                                         const float* __restrict__ ref,
                                                                         const float* __restrict__ base,
                                                                         const long* __restrict__ tracks,
                                                                         double voicing, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[kCounts][kThreads];
  const int tid = threadIdx.x;
  const long* m = tracks + (long)blockIdx.x * M_K;
  const long n = m[M_N], nf = base ? m[M_NFLIP] : 0;
  const float* p = pred + m[M_POFF];
  const float* f = ref + m[M_ROFF];
  int c[kCounts] = {0, 0, 0, 0, 0, 0};          // voiced, rpa, rca, octave, vuv agreements, flips
  for (long i = tid; i < n; i += kThreads) {
    const bool rv = f[i] > 0.f, pv = (double)p[i] > voicing;
    c[4] += rv == pv;
    if (rv) {
      c[0] += 1;
      const double pc = 1200.0 * log2((double)fmaxf(p[i], 1e-5f) / 55.0), rc = 1200.0 * log2((double)f[i] / 55.0);
      const double d = pc - rc;
      c[1] += fabs(d) <= 50.0;
      double w = fmod(d + 600.0, 1200.0);
      if (w < 0.0) w += 1200.0;
      c[2] += fabs(w - 600.0) <= 50.0;
      const double oct = rint(d / 1200.0);
      c[3] += fabs(d) > 50.0 && oct != 0.0 && fabs(d - oct * 1200.0) <= 50.0;
    }
  }
  if (nf > 0) {
    const float* bl = base + m[M_BOFF];
    for (long i = tid; i < nf; i += kThreads) c[5] += ((double)bl[i] > voicing) != ((double)p[i] > voicing);
  }
  for (int k = 0; k < kCounts; ++k) s_cnt[k][tid] = c[k];
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int k = 0; k < kCounts; ++k) s_cnt[k][tid] += s_cnt[k][tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double nv = (double)s_cnt[0][0];
    double* o = out + (long)blockIdx.x * 7;
    o[0] = nv > 0 ? (double)s_cnt[1][0] / nv : nan;
    o[1] = nv > 0 ? (double)s_cnt[2][0] / nv : nan;
    o[2] = (double)s_cnt[4][0] / (double)(n > 1 ? n : 1);
    o[3] = nv > 0 ? (double)s_cnt[3][0] / nv : nan;
    o[4] = nf > 0 ? (double)s_cnt[5][0] / (double)nf : nan;
    o[5] = nv;
    o[6] = (double)n;
  }
}

}  // namespace

extern "C" int pe_stress_plan_fields(void) { return S_K; }

/* Host-only layout; see include/pitchextractor_hip.h. */
extern "C" int pe_stress_plan(int n_rows, const long* n, const long* x_off, const long* y_off, long* consts4, long* meta,
                              long* totals2) {
  if (!consts4 || !totals2 || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows > 0 && (!n || !x_off || !y_off || !meta)) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (n[r] < 0 || n[r] > kMaxSamples || x_off[r] < 0 || y_off[r] < 0) return PE_E_ARG;
  consts4[0] = kStep; consts4[1] = kTableFloats; consts4[2] = kPiece; consts4[3] = kClipChunk;
  long s = 0, b = 0;
  for (int r = 0; r < n_rows; ++r) {
    long* m = meta + (long)r * S_K;
    m[S_XOFF] = x_off[r]; m[S_N] = n[r]; m[S_YOFF] = y_off[r]; m[S_SOFF] = s;
    m[S_BLOCKS] = (n[r] + kStep - 1) / kStep; m[S_BOFF] = b;
    s += n[r]; b += m[S_BLOCKS];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_BLOCKS] = b;
  return PE_OK;
}

extern "C" size_t pe_stress_rir_workspace_bytes(long blocks) {
  return blocks > 0 ? (size_t)blocks * (kC * sizeof(float2) + sizeof(float)) : 0;
}

extern "C" int pe_stress_spectra(const float* x, const long* meta, const long* host_meta, int n_rows, int partition,
                                 const float* tables, long n_table, float* spectra, void* stream) {
  long tot[2];
  if (partition != 0 && partition != 1) return PE_E_ARG;
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!x || !meta || !tables || !spectra || n_table != kTableFloats) return PE_E_ARG;
  hipLaunchKernelGGL(stress_spectra_kernel, dim3(grid_of(tot[TOT_BLOCKS])), dim3(kThreads), 0, pe_stream(stream), x,
                     meta, tables, n_rows, tot[TOT_BLOCKS], partition, reinterpret_cast<float2*>(spectra));
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stress_rir(const float* x, const long* meta, const long* host_meta, int n_rows,
                             const float* rir_spectra, const long* rir_meta, const long* host_rir_meta, int n_rirs,
                             const int* rir_index, const int* host_rir_index, const float* tables, long n_table, float* y,
                             void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2], rtot[2];
  const int st = open_batch(n_rows, host_meta, tot);
  if (st != PE_OK && st != kNothing) return st;
  if (n_rirs < 1 || n_rirs > kMaxRows || !host_rir_meta || !meta_ok(host_rir_meta, n_rirs, rtot)) return PE_E_ARG;
  for (int k = 0; k < n_rirs; ++k)
    if (host_rir_meta[(long)k * S_K + S_N] < 1) return PE_E_ARG;
  if (n_rows > 0 && !host_rir_index) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (host_rir_index[r] < 0 || host_rir_index[r] >= n_rirs) return PE_E_ARG;
  if (st == kNothing) return PE_OK;
  if (!x || !meta || !rir_spectra || !rir_meta || !rir_index || !tables || !y || n_table != kTableFloats)
    return PE_E_ARG;
  const long blocks = tot[TOT_BLOCKS];
  if (!workspace || workspace_bytes < pe_stress_rir_workspace_bytes(blocks)) return PE_E_WORKSPACE;
  float2* xs = static_cast<float2*>(workspace);
  float* peak = reinterpret_cast<float*>(xs + blocks * kC);
  const dim3 grid(grid_of(blocks)), wg(kThreads);
  hipLaunchKernelGGL(stress_spectra_kernel, grid, wg, 0, pe_stream(stream), x, meta, tables, n_rows, blocks, 0, xs);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(stress_rir_convolve_kernel, grid, wg, 0, pe_stream(stream), xs, meta,
                     reinterpret_cast<const float2*>(rir_spectra), rir_meta, rir_index, tables, n_rows, blocks, y, peak);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(stress_rir_normalize_kernel, grid, wg, 0, pe_stream(stream), meta, peak, n_rows, blocks, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stress_biquad(const float* x, const long* meta, const long* host_meta, int n_rows,
                                const double* coeffs, int n_stages, float* y, void* stream) {
  long tot[2];
  if (!coeffs || n_stages < 1 || n_stages > kMaxStages) return PE_E_ARG;
  Biquads K;
  memset(&K, 0, sizeof(K));
  K.stages = n_stages;
  for (int s = 0; s < n_stages; ++s) {
    for (int j = 0; j < 5; ++j) {
      if (!isfinite(coeffs[5 * s + j])) return PE_E_ARG;
      K.c[s][j] = coeffs[5 * s + j];
    }
    // poles inside the unit circle: the stability triangle |a2| < 1, |a1| < 1 + a2
    const double a1 = K.c[s][3], a2 = K.c[s][4];
    if (!(fabs(a2) < 1.0) || !(fabs(a1) < 1.0 + a2)) return PE_E_UNSUPPORTED;
  }
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!x || !meta || !y) return PE_E_ARG;
  hipLaunchKernelGGL(stress_biquad_kernel, dim3(n_rows), dim3(64), 0, pe_stream(stream), x, meta, K, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stress_clip(const float* x, const long* meta, const long* host_meta, int n_rows, double q, int copy,
                              float* y, float* thresholds, void* stream) {
  long tot[2];
  if (!copy && !(q >= 0.0 && q <= 1.0)) return PE_E_ARG;
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!x || !meta || !y) return PE_E_ARG;
  hipLaunchKernelGGL(stress_clip_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), x, meta, (float)q,
                     copy ? 1 : 0, nullptr, nullptr, y, thresholds);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stress_clip_rows(const float* x, const long* meta, const long* host_meta, int n_rows, const double* q,
                                   const double* host_q, const int* copy, const int* host_copy, float* y,
                                   float* thresholds, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!host_q || !host_copy) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (!host_copy[r] && !(host_q[r] >= 0.0 && host_q[r] <= 1.0)) return PE_E_ARG;
  if (!x || !meta || !q || !copy || !y) return PE_E_ARG;
  hipLaunchKernelGGL(stress_clip_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), x, meta, 0.f, 0, q, copy, y,
                     thresholds);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" size_t pe_stress_agc_workspace_bytes(long samples) {
  return samples > 0 ? (size_t)samples * sizeof(float) : 0;
}

extern "C" int pe_stress_agc(const float* x, const long* meta, const long* host_meta, int n_rows, const double* params4,
                             int smoothing, float* y, void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2];
  if (!params4 || smoothing < 0 || smoothing > (1 << 13)) return PE_E_ARG;
  for (int j = 0; j < 4; ++j)
    if (!isfinite(params4[j])) return PE_E_ARG;
  AgcParams P{params4[0], params4[1], params4[2], params4[3], smoothing};
  if (!(P.attack > 0.0 && P.attack < 1.0) || !(P.release > 0.0 && P.release < 1.0) || !(P.target > 0.0)) return PE_E_ARG;
  if (!(P.max_gain >= 1.0) || !(P.max_gain < 256.0)) return PE_E_ARG;        // the exact window sums need < 2^8
  const int st = open_batch(n_rows, host_meta, tot);
  if (st != PE_OK && st != kNothing) return st;
  if (smoothing > 1)
    for (int r = 0; r < n_rows; ++r)
      if (host_meta[(long)r * S_K + S_N] < smoothing) return PE_E_ARG;       // np.convolve would return `smoothing` samples
  if (st == kNothing) return PE_OK;
  if (!x || !meta || !y) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_stress_agc_workspace_bytes(tot[TOT_SAMPLES])) return PE_E_WORKSPACE;
  float* gains = static_cast<float*>(workspace);
  hipLaunchKernelGGL(stress_agc_walk_kernel, dim3(n_rows), dim3(64), 0, pe_stream(stream), x, meta, P, gains);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(stress_agc_apply_kernel, dim3(grid_of(tot[TOT_BLOCKS])), dim3(kThreads), 0, pe_stream(stream), x,
                     meta, gains, n_rows, tot[TOT_BLOCKS], smoothing, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_melody_metrics_fields(void) { return M_K; }

extern "C" int pe_melody_metrics(const float* f0_pred, const float* f0_ref, const float* f0_base, const long* tracks,
                                 const long* host_tracks, int n_rows, double voicing_threshold_hz, double* out7,
                                 void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || !isfinite(voicing_threshold_hz)) return PE_E_ARG;
  if (n_rows == 0) return PE_OK;
  if (!host_tracks) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = host_tracks + (long)r * M_K;
    if (m[M_POFF] < 0 || m[M_N] < 0 || m[M_ROFF] < 0 || m[M_BOFF] < 0 || m[M_NFLIP] < 0) return PE_E_ARG;
  }
  if (!f0_pred || !f0_ref || !tracks || !out7) return PE_E_ARG;
  hipLaunchKernelGGL(stress_melody_metrics_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), f0_pred, f0_ref,
                     f0_base, tracks, voicing_threshold_hz, out7);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
