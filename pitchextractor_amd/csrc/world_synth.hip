// WORLD vocoder synthesis on the GPU: WORLD's Synthesis (pyworld 0.3.x `synthesize`) for ragged batches, as the
// reference's synthetic-data generator calls it (Utils/synthetic.py:194-220) -- one minimum-phase impulse response of
// N = fft_size samples per glottal pulse, overlap-added.  The time base (pulse positions from the running phase of the
// interpolated F0) is a sequential float64 recurrence whose rounding decides where a pulse falls whenever a period is a
// whole number of samples; it stays on the host (pitchextractor_amd/world.py) and the device gets the finished pulse
// table.  pe_world_plan (host only) lays the batch out and keeps only the pulses whose response overlaps a row's
// output window.
//
//   1. Responses: one workgroup per planned pulse, everything in LDS with the shared N-point FFT (fft_lds, dsp.h).
//      The envelope S and the squared aperiodicity A are interpolated between the pulse's two frames.  The two
//      minimum-phase spectra (periodic: amplitude S (1 - A); aperiodic: S A, or S for an unvoiced pulse) share their
//      transforms: the two real, even half-log spectra travel as the real and the imaginary part of one sequence, whose
//      inverse transform is cepstrum_p + i cepstrum_a; both are folded and one forward transform gives F_p + i F_a,
//      which the Hermitian split separates again.  The pulse's noise segment (given, or Philox + Box-Muller) is
//      transformed once; the periodic spectrum (times the fractional-delay ramp) and the aperiodic one (times the noise
//      spectrum) again share one inverse transform as its real and imaginary part.  Four N-point transforms per pulse.
//   2. Overlap-add in gather form: one thread per output sample finds the pulses covering it by binary search in the
//      row's planned pulse list and adds their responses in ascending pulse order -- no atomics, so a row is
//      bit-identical alone and in any batch.  Gain, optional additive noise and the write into the caller's batch row
//      are the epilogue.
#include <math.h>
#include "common.h"
#include "world_frames.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;

// per-row plan fields (int64); see pe_world_plan
enum {
  W_L, W_YLEN, W_PCNT, W_POFF, W_SPOFF, W_SPSTRIDE, W_APOFF, W_APSTRIDE, W_NOFF, W_SEED, W_JLO, W_JCNT, W_JOFF,
  W_OOFF, W_K
};
// per planned pulse (int64 x 6, double x 2)
enum { P_INDEX, P_LO, P_HI, P_NS, P_VOICED, P_ROW, P_K };
enum { F_FRAC, F_SHIFT, F_K };

__device__ __forceinline__ float2 cexp2(float2 z) {           // exp(z), full-accuracy exp / sin / cos
  float s, c;
  sincosf(z.y, &s, &c);
  const float e = expf(z.x);
  return make_float2(e * c, e * s);
}

template <int LOG2N>
__global__ __launch_bounds__(kThreads) void world_responses_kernel(
    const float* __restrict__ sp, const float* __restrict__ ap, const float* __restrict__ noise,
    const long* __restrict__ meta, const long* __restrict__ pulses, const double* __restrict__ pulse_f,
    const float* __restrict__ table, long n_pulses, float* __restrict__ resp) {
  constexpr int N = 1 << LOG2N, H = N / 2;
  __shared__ float2 s_tw[N];
  __shared__ float2 s_buf[N];
  __shared__ float2 s_z[N];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  for (int m = tid; m < N; m += kThreads) s_tw[m] = reinterpret_cast<const float2*>(table)[m];
  const float* dcr = table + 2 * N;
  __syncthreads();
  for (long g = blockIdx.x; g < n_pulses; g += gridDim.x) {
    const long* pu = pulses + g * P_K;
    const long* m = meta + pu[P_ROW] * W_K;
    const long index = pu[P_INDEX];
    const int ns = (int)pu[P_NS];
    const bool voiced = pu[P_VOICED] != 0;
    const bool two = pu[P_LO] != pu[P_HI];
    const float frac = (float)pulse_f[g * F_K + F_FRAC];
    const double shift = pulse_f[g * F_K + F_SHIFT];            // shift * fs in [0, 1]
    const float* s_lo = sp + m[W_SPOFF] + pu[P_LO] * m[W_SPSTRIDE];
    const float* s_hi = sp + m[W_SPOFF] + pu[P_HI] * m[W_SPSTRIDE];
    const bool has_ap = m[W_APOFF] >= 0;
    const float* a_lo = has_ap ? ap + m[W_APOFF] + pu[P_LO] * m[W_APSTRIDE] : nullptr;
    const float* a_hi = has_ap ? ap + m[W_APOFF] + pu[P_HI] * m[W_APSTRIDE] : nullptr;
    auto env = [&](int k) {
      const float a = fabsf(s_lo[k]);
      return two ? (1.f - frac) * a + frac * fabsf(s_hi[k]) : a;
    };
    // clip(ap, 0.001, 1)^2 (0.999999999999 is 1 in float32); no ap = zeros, through the same arithmetic
    auto aper = [&](int k) {
      float a = fminf(fmaxf(has_ap ? a_lo[k] : 0.f, 0.001f), 1.0f);
      a *= a;
      if (two) {
        float b = fminf(fmaxf(has_ap ? a_hi[k] : 0.f, 0.001f), 1.0f);
        b *= b;
        a = (1.f - frac) * a + frac * b;
      }
      return a;
    };
    const bool periodic = voiced && !(aper(0) > 0.999f);

    // noise segment, its mean removed, zero padded; its transform stays in s_z
    float zv[N / kThreads];
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < N / kThreads; ++q) {
      const int j = tid + kThreads * q;
      float v = 0.f;
      if (j < ns) v = m[W_NOFF] >= 0 ? noise[m[W_NOFF] + index + j] : world_randn((uint64_t)m[W_SEED], (uint64_t)(index + j));
      zv[q] = v;
      part += v;
    }
    const float mean = ns > 0 ? block_sum(part, s_red, tid) / (float)ns : 0.f;
#pragma unroll
    for (int q = 0; q < N / kThreads; ++q) {
      const int j = tid + kThreads * q;
      s_z[j] = make_float2(j < ns ? zv[q] - mean : 0.f, 0.f);
    }
    // half log amplitudes of the two spectra as real + i imaginary, mirrored to N points
    for (int k = tid; k <= H; k += kThreads) {
      const float S = env(k), A = aper(k);
      const float lp = periodic ? 0.5f * logf(S * (1.f - A) + 1e-12f) : 0.f;
      const float la = 0.5f * logf(voiced ? S * A : S);
      s_buf[k] = make_float2(lp, la);
      if (k > 0 && k < H) s_buf[N - k] = make_float2(lp, la);
    }
    __syncthreads();
    fft_lds<LOG2N, false, kThreads>(s_z, s_tw, tid);
    fft_lds<LOG2N, true, kThreads>(s_buf, s_tw, tid);           // N x the two real cepstra
    {
      float2 c[N / kThreads];
#pragma unroll
      for (int q = 0; q < N / kThreads; ++q) {
        const int j = tid + kThreads * q;
        const float w = (j == 0 || j == H) ? 1.f / N : (j < H ? 2.f / N : 0.f);
        const float2 v = s_buf[j];
        c[q] = make_float2(v.x * w, v.y * w);
      }
#pragma unroll
      for (int q = 0; q < N / kThreads; ++q) s_buf[tid + kThreads * q] = c[q];   // own elements only: no barrier between
    }
    __syncthreads();
    fft_lds<LOG2N, false, kThreads>(s_buf, s_tw, tid);          // F_p + i F_a
    {
      constexpr int NK = H / kThreads + 1;
      float2 P[NK], Q[NK];
#pragma unroll
      for (int q = 0; q < NK; ++q) {
        const int k = tid + kThreads * q;
        if (k > H) break;
        const float2 xk = s_buf[k], xc = conj2(s_buf[(N - k) & (N - 1)]);
        float2 fp, fa;
        real_fft_split(xk, xc, fp, fa);                          // fp = (xk + xc) / 2, fa = (xk - xc) / 2i
        float2 hp = make_float2(0.f, 0.f);
        if (periodic) {
          float rs, rc;
          sincospif((float)(-2.0 * shift * (double)k / (double)N), &rs, &rc);     // argument in [-pi, 0]
          hp = cmul(cexp2(fp), make_float2(rc, rs));
        }
        float2 ha = cmul(cexp2(fa), s_z[k]);
        if (k == 0 || k == H) { hp.y = 0.f; ha.y = 0.f; }         // the inverse real transform drops them
        P[q] = hp; Q[q] = ha;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NK; ++q) {
        const int k = tid + kThreads * q;
        if (k > H) break;
        s_buf[k] = make_float2(P[q].x - Q[q].y, P[q].y + Q[q].x);               // P + i Q
        if (k > 0 && k < H) s_buf[N - k] = make_float2(P[q].x + Q[q].y, Q[q].x - P[q].y);   // conj(P) + i conj(Q)
      }
    }
    __syncthreads();
    fft_lds<LOG2N, true, kThreads>(s_buf, s_tw, tid);           // real: periodic response, imaginary: aperiodic
    // fftshift, DC removal over the causal half, sum
    float dpart = 0.f;
    for (int j = tid; j < H; j += kThreads) dpart += s_buf[j].x;
    const float dc = block_sum(dpart, s_red, tid);
    const float root = sqrtf((float)ns);
    float* out = resp + g * N;
#pragma unroll
    for (int q = 0; q < N / kThreads; ++q) {
      const int j = tid + kThreads * q;
      const float2 v = s_buf[(j + H) & (N - 1)];
      const float per = periodic ? (j >= H ? v.x : 0.f) - dc * dcr[j] : 0.f;
      out[j] = (per * root + v.y) * (1.f / N);
    }
    __syncthreads();                                            // s_buf / s_z reads done before the next pulse
  }
}

template <int LOG2N>
__global__ __launch_bounds__(kThreads) void world_ola_kernel(const float* __restrict__ resp,
                                                             const long* __restrict__ meta,
                                                             const long* __restrict__ pulses,
                                                             const float* __restrict__ gains,
                                                             const float* __restrict__ out_noise, int n_rows,
                                                             long total, float* __restrict__ out) {
  constexpr int N = 1 << LOG2N, H = N / 2;
  for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long)gridDim.x * kThreads) {
    const int row = find_row(meta, n_rows, W_K, W_JOFF, g);
    const long* m = meta + (long)row * W_K;
    const long i = m[W_JLO] + (g - m[W_JOFF]);
    const long p0 = m[W_POFF], cnt = m[W_PCNT];
    // first planned pulse with index >= i - H; pulse p covers samples index - H + 1 .. index + H
    long lo = 0, hi = cnt;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (pulses[(p0 + mid) * P_K + P_INDEX] < i - H) lo = mid + 1; else hi = mid;
    }
    float acc = 0.f;
    for (long p = lo; p < cnt; ++p) {
      const long idx = pulses[(p0 + p) * P_K + P_INDEX];
      if (idx > i + H - 1) break;
      acc += resp[(p0 + p) * N + (i - idx + H - 1)];
    }
    float y = acc * gains[row];
    if (out_noise) y += out_noise[g];
    out[m[W_OOFF] + (g - m[W_JOFF])] = y;
  }
}

}  // namespace

extern "C" int pe_world_plan_fields(void) { return W_K; }

/* Host-only batch layout; see include/pitchextractor_hip.h. */
extern "C" int pe_world_plan(int n_rows, const long* n_frames, const double* f0, const long* pulse_cnt,
                             const long* index, const double* shift, const unsigned char* voiced, const long* sp_off,
                             const long* sp_stride, const long* ap_off, const long* ap_stride, const long* noise_off,
                             const long* seeds, const long* j_lo, const long* j_cnt, const long* out_row,
                             long out_stride, double fs, double frame_period_ms, int fft_size, long* meta,
                             long* pulses, double* pulse_f, long* totals) {
  if (fft_size <= 0 || (fft_size & (fft_size - 1))) return PE_E_ARG;
  if (!world_fft_size_ok(fft_size)) return PE_E_UNSUPPORTED;
  if (n_rows < 0 || n_rows > kMaxRows || !totals || !(fs > 0.0) || !(frame_period_ms > 0.0) || !isfinite(fs) ||
      !isfinite(frame_period_ms))
    return PE_E_ARG;
  if (n_rows > 0 && (!n_frames || !pulse_cnt || !sp_off || !sp_stride || !j_lo || !j_cnt || !out_row || !meta))
    return PE_E_ARG;
  const long N = fft_size, H = N / 2, bins = H + 1;
  const double fp = frame_period_ms / 1000.0;
  long f_off = 0, t_off = 0, p_tot = 0, j_tot = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long L = n_frames[r], P = pulse_cnt[r];
    if (L < 1 || L > (1L << 31) || P < 0 || (P > 0 && (!index || !shift || !voiced || !pulses || !pulse_f)))
      return PE_E_ARG;
    const long y_len = (long)((double)L * frame_period_ms * fs / 1000.0);
    if (y_len > (1L << 31) || sp_off[r] < 0 || sp_stride[r] < 0 || (sp_stride[r] > 0 && sp_stride[r] < bins) ||
        j_lo[r] < 0 || j_cnt[r] < 0 || j_lo[r] + j_cnt[r] > y_len || out_row[r] < 0 || out_stride < j_cnt[r])
      return PE_E_ARG;
    const bool has_ap = ap_off && ap_off[r] >= 0;
    if (has_ap && (!ap_stride || ap_stride[r] < 0 || (ap_stride[r] > 0 && ap_stride[r] < bins))) return PE_E_ARG;
    if (f0)
      for (long i = 0; i < L; ++i)
        if (!isfinite(f0[f_off + i])) return PE_E_ARG;
    const long* idx = index + t_off;
    for (long p = 0; p < P; ++p) {
      const double sf = shift[t_off + p] * fs;
      if (idx[p] < 0 || idx[p] >= y_len || (p > 0 && idx[p] <= idx[p - 1]) || !(sf >= 0.0 && sf <= 1.0))
        return PE_E_ARG;
      if (p + 1 < P && idx[p + 1] - idx[p] > N) return PE_E_ARG;      // a noise segment longer than the transform
    }
    // pulses whose N-sample response [index - H + 1, index + H] meets the window
    long first = 0, count = 0;
    if (j_cnt[r] > 0) {
      const long lo_i = j_lo[r] - H, hi_i = j_lo[r] + j_cnt[r] - 1 + H - 1;
      while (first < P && idx[first] < lo_i) ++first;
      while (first + count < P && idx[first + count] <= hi_i) ++count;
    }
    for (long q = 0; q < count; ++q) {
      const long p = first + q;
      const double pos = ((double)idx[p] / fs) / fp;
      const double fl = floor(pos);
      long* pu = pulses + (p_tot + q) * P_K;
      pu[P_INDEX] = idx[p];
      pu[P_LO] = min(L - 1, (long)fl);
      pu[P_HI] = min(L - 1, (long)ceil(pos));
      pu[P_NS] = p + 1 < P ? idx[p + 1] - idx[p] : 0;
      pu[P_VOICED] = voiced[t_off + p] ? 1 : 0;
      pu[P_ROW] = r;
      pulse_f[(p_tot + q) * F_K + F_FRAC] = pos - fl;
      pulse_f[(p_tot + q) * F_K + F_SHIFT] = shift[t_off + p] * fs;
    }
    long* m = meta + (long)r * W_K;
    m[W_L] = L; m[W_YLEN] = y_len; m[W_PCNT] = count; m[W_POFF] = p_tot; m[W_SPOFF] = sp_off[r];
    m[W_SPSTRIDE] = sp_stride[r]; m[W_APOFF] = has_ap ? ap_off[r] : -1; m[W_APSTRIDE] = has_ap ? ap_stride[r] : 0;
    m[W_NOFF] = noise_off && noise_off[r] >= 0 ? noise_off[r] : -1; m[W_SEED] = seeds ? seeds[r] : 0;
    m[W_JLO] = j_lo[r]; m[W_JCNT] = j_cnt[r]; m[W_JOFF] = j_tot; m[W_OOFF] = out_row[r] * out_stride;
    f_off += L; t_off += P; p_tot += count; j_tot += j_cnt[r];
  }
  totals[0] = p_tot; totals[1] = j_tot;
  return PE_OK;
}

extern "C" int pe_world_responses(const float* sp, const float* ap, const float* noise, const long* meta,
                                  const long* pulses, const double* pulse_f, const float* table, int n_rows,
                                  long n_pulses, int fft_size, float* responses, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_pulses < 0 || fft_size <= 0) return PE_E_ARG;
  if (!world_fft_size_ok(fft_size)) return PE_E_UNSUPPORTED;
  if (n_pulses == 0 || n_rows == 0) return PE_OK;
  if (!sp || !meta || !pulses || !pulse_f || !table || !responses) return PE_E_ARG;
  const dim3 grid(grid_for(n_pulses, 1, 8192)), block(kThreads);
  return with_log2<9, 11>(__builtin_ctz(fft_size), [&](auto L) {
    hipLaunchKernelGGL(world_responses_kernel<decltype(L)::value>, grid, block, 0, pe_stream(stream), sp, ap, noise,
                       meta, pulses, pulse_f, table, n_pulses, responses);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}

extern "C" int pe_world_overlap_add(const float* responses, const long* meta, const long* pulses, const float* gains,
                                    const float* out_noise, int n_rows, long n_out, int fft_size, float* out,
                                    void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || n_out < 0 || fft_size <= 0) return PE_E_ARG;
  if (!world_fft_size_ok(fft_size)) return PE_E_UNSUPPORTED;
  if (n_out == 0 || n_rows == 0) return PE_OK;
  if (!meta || !gains || !out) return PE_E_ARG;               // responses / pulses may be empty: a window no pulse meets
  const dim3 grid(grid_for(n_out, kThreads, 8192)), block(kThreads);
  return with_log2<9, 11>(__builtin_ctz(fft_size), [&](auto L) {
    hipLaunchKernelGGL(world_ola_kernel<decltype(L)::value>, grid, block, 0, pe_stream(stream), responses, meta, pulses,
                       gains, out_noise, n_rows, n_out, out);
    PE_LAUNCH_CHECK();
    return PE_OK;
  });
}
