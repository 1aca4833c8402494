// Synthesized evaluation stimuli of the reference's notebooks (Utils/dynamic_pitch_behavior.ipynb through
// Utils/dynamic_pitch_tools.py, Utils/pitch_range_and_timbre_coverage.ipynb) on ragged batches: sinusoids that follow a
// glide, a vibrato or a given F0 curve, harmonic tones, the raised-cosine fade, the noise mix and the peak
// normalisation, the analytic reference at frame rate, and the dynamic metrics (RMS cents, tracking lag, overshoot,
// final error).  Pinned by the float64 restatement in tests/stimuli_ref.py.
//
// pe_stim_plan (host only) lays the rows out: offset and length (the shared row header), kind, sample prefix, the
// row's pieces of kPiece samples counted from the row's own first sample and their prefix, the given curve, the
// partial count, the fade length and the noise; and a table of doubles per row with every derived parameter, each
// evaluated once on the host in the reference's order.  Every stage is a fixed number of launches whatever the rows:
//   phase:     piece sums (one workgroup per piece: a thread sums its kRun samples in order, the threads are scanned),
//              carries (one thread per row walks the row's piece sums in order), phases (the piece scan again, plus the
//              carry).  Three launches, and no workgroup waits on another.
//   synth:     float32(amplitude sin(phase)).
//   tone:      the sum of up to 16 partials in the profile's order.
//   finish:    the mix at an SNR of snr_mix.h in place, under the fade (fade and piece sums of squares, row rms and
//              scale, noise mix and piece peaks, row peak with the normalisation), which pe_noise_mix runs too.  Four.
//   reference: one thread per frame: the bracketing samples of the float32 time axis, np.interp's expression.
//   metrics:   one workgroup per row; every lag of the full cross-correlation is summed by one thread in index order.
// Everything is double with contraction off; nothing a row computes depends on where the row lies or on its
// neighbours: a row's result is the same alone, packed at an odd offset or padded.
#include <math.h>
#include "common.h"
#include "snr_mix.h"

using namespace pe;

namespace {

constexpr int kMaxPartials = 16;
constexpr long kMaxSamples = (1L << 31) - 8;
constexpr double kTwoPi = 2.0 * 3.141592653589793;
constexpr double kFadeTime = 0.02;

enum { K_CURVE, K_GLIDE, K_VIBRATO, K_TONE, K_KINDS };
enum { S_OFF, S_N, S_KIND, S_SOFF, S_PIECES, S_POFF, S_COFF, S_CLEN, S_NPART, S_FADE, S_NOFF, S_K };
static_assert(S_OFF == kRowOffset && S_N == kRowLength, "the plan opens with the shared row header");
enum { TOT_SAMPLES, TOT_PIECES };
// doubles per row: amplitude; a, b, c of the kind (glide: start, step, end; vibrato: base, depth / 1200, 2 pi rate;
// tone and constant curve: the frequency); snr_db; sr; the time step duration / n; then {amplitude, 2 pi f h} per partial
enum { P_AMP, P_A, P_B, P_C, P_SNR, P_SR, P_TSTEP, P_SPARE, P_PARTIALS, P_K = P_PARTIALS + 2 * kMaxPartials };
enum { F_FOFF, F_NF, F_K };                      // frame table of pe_stim_reference: frame prefix, frames
enum { M_POFF, M_N, M_ROFF, M_K };               // tracks of pe_dynamic_metrics: pred offset, frames, ref offset
static_assert(F_FOFF == kRowOffset && F_NF == kRowLength && M_POFF == kRowOffset && M_N == kRowLength, "row header");

// The plan as snr_mix.h reads it: in place under the fade, packed noise that a row may lack, snr_db in the row's
// parameters; rows of a few dozen pieces, so the division finds the row peaks itself.
struct StimMixRows {
  static constexpr int kFields = S_K, kPieceOffset = S_POFF, kFade = S_FADE, kNoiseOffset = S_NOFF, kSnrStride = P_K;
  static constexpr bool kInPlace = true, kPeakLaunch = false;
};

long fade_samples(double sr) { return (long)fmax(kFadeTime * sr, 0.0); }

bool meta_ok(const long* hm, int n_rows, long* totals2) {
  long s = 0, p = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * S_K;
    if (m[S_N] < 1 || m[S_N] > kMaxSamples || m[S_OFF] < 0 || m[S_KIND] < 0 || m[S_KIND] >= K_KINDS) return false;
    if (m[S_PIECES] != (m[S_N] + kPiece - 1) / kPiece || m[S_SOFF] != s || m[S_POFF] != p) return false;
    if (m[S_FADE] < 0 || (m[S_FADE] > 0 && m[S_N] < m[S_FADE])) return false;
    if (m[S_NPART] < 0 || m[S_NPART] > kMaxPartials || m[S_NOFF] < -1) return false;
    if (m[S_KIND] == K_CURVE && (m[S_COFF] < 0 || (m[S_CLEN] != 1 && m[S_CLEN] != m[S_N]))) return false;
    s += m[S_N]; p += m[S_PIECES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_PIECES] = p;
  return true;
}

int open_batch(int n_rows, const long* host_meta, long* totals2) {
  return open_rows(n_rows, PE_OK, host_meta, [&] { return meta_ok(host_meta, n_rows, totals2); },
                   &totals2[TOT_SAMPLES]);
}

// Sample i of the row's F0 curve in double, as the reference's NumPy expressions give it.
__device__ __forceinline__ double curve_at(const long* m, const double* p, const float* __restrict__ curves, long i) {
#pragma clang fp contract(off)
  const long kind = m[S_KIND], n = m[S_N];
  if (kind == K_GLIDE) return (n > 1 && i == n - 1) ? p[P_C] : (double)i * p[P_B] + p[P_A];
  if (kind == K_VIBRATO) {
    const double t = (double)i * p[P_TSTEP];
    return p[P_A] * exp2(p[P_B] * sin(p[P_C] * t));
  }
  if (kind == K_CURVE) return (double)curves[m[S_COFF] + (m[S_CLEN] == 1 ? 0 : i)];
  return (double)(float)p[P_A];
}

// ---- phase ---------------------------------------------------------------------------------------------------------
// Piece g of a curve row: omega[i] = ((2 pi) curve[i]) / sr; thread t owns samples [t kRun, (t + 1) kRun) of the piece.
// WRITE == false: sums[g] = the piece's sum.  WRITE == true: phase[sample prefix + i] = carry[g] + (the sum of the
// threads before) + (the thread's running sum): the same additions whatever the batch around the row.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void stim_phase_kernel(const long* __restrict__ meta,
                                                              const double* __restrict__ prm,
                                                              const float* __restrict__ curves, int n_rows, long pieces,
                                                              double* __restrict__ sums, double* __restrict__ phase) {
#pragma clang fp contract(off)
  __shared__ double s_sum[kThreads];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_POFF, g);
    const long* m = meta + (long)row * S_K;
    if (m[S_KIND] == K_TONE) continue;                        // uniform over the workgroup
    const double* p = prm + (long)row * P_K;
    const long n = m[S_N], i0 = (g - m[S_POFF]) * kPiece + (long)tid * kRun;
    double w[kRun], local = 0.0;
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      w[u] = i0 + u < n ? (kTwoPi * curve_at(m, p, curves, i0 + u)) / p[P_SR] : 0.0;
      local += w[u];
    }
    double total;
    const double before = block_scan(local, s_sum, tid, total);
    if (!WRITE) {
      if (tid == 0) sums[g] = total;
    } else {
      double run = sums[g] + before;
      double* out = phase + m[S_SOFF];
#pragma unroll
      for (int u = 0; u < kRun; ++u)
        if (i0 + u < n) { run += w[u]; out[i0 + u] = run; }
    }
  }
}

// sums[piece prefix + k] -> the sum of the row's pieces before k, in order (one thread per row)
__global__ __launch_bounds__(kThreads) void stim_carry_kernel(const long* __restrict__ meta, int n_rows,
                                                              double* __restrict__ sums) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * kThreads + threadIdx.x;
  if (row >= n_rows) return;
  const long* m = meta + (long)row * S_K;
  if (m[S_KIND] == K_TONE) return;
  double* s = sums + m[S_POFF];
  double carry = 0.0;
  for (long k = 0; k < m[S_PIECES]; ++k) {
    const double v = s[k];
    s[k] = carry;
    carry += v;
  }
}

__global__ __launch_bounds__(kThreads) void stim_synth_kernel(const long* __restrict__ meta,
                                                              const double* __restrict__ prm,
                                                              const double* __restrict__ phase, int n_rows, long pieces,
                                                              float* __restrict__ y) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_POFF, g);
    const long* m = meta + (long)row * S_K;
    if (m[S_KIND] == K_TONE) continue;
    const double amp = prm[(long)row * P_K + P_AMP];
    const long n = m[S_N], base = (g - m[S_POFF]) * kPiece;
    const double* ph = phase + m[S_SOFF];
    float* out = y + m[S_OFF];
    for (int j = tid; j < kPiece && base + j < n; j += kThreads) out[base + j] = (float)(amp * sin(ph[base + j]));
  }
}

// ---- harmonic tones ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void stim_tone_kernel(const long* __restrict__ meta,
                                                             const double* __restrict__ prm, int n_rows, long pieces,
                                                             float* __restrict__ y) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, S_K, S_POFF, g);
    const long* m = meta + (long)row * S_K;
    if (m[S_KIND] != K_TONE) continue;
    const double* p = prm + (long)row * P_K;
    const int parts = (int)m[S_NPART];
    const long n = m[S_N], base = (g - m[S_POFF]) * kPiece;
    float* out = y + m[S_OFF];
    for (int j = tid; j < kPiece && base + j < n; j += kThreads) {
      const double t = (double)(base + j) * p[P_TSTEP];
      double acc = 0.0;
      for (int h = 0; h < parts; ++h) acc += p[P_PARTIALS + 2 * h] * sin(p[P_PARTIALS + 2 * h + 1] * t);
      out[base + j] = (float)acc;
    }
  }
}

// ---- reference at frame rate ---------------------------------------------------------------------------------------
// ref[f] = float32(np.interp(tau[f], float32(t), float32(curve))) with t[i] = i tstep: j with t32[j] <= tau < t32[j + 1]
// from floor(tau / tstep) corrected against the rounded times; the last sample at or beyond t32[n - 1].
__global__ __launch_bounds__(kThreads) void stim_reference_kernel(const long* __restrict__ meta,
                                                                  const double* __restrict__ prm,
                                                                  const float* __restrict__ curves,
                                                                  const long* __restrict__ ftab,
                                                                  const double* __restrict__ tau, int n_rows,
                                                                  long frames, float* __restrict__ ref) {
#pragma clang fp contract(off)
  for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < frames; f += (long)gridDim.x * kThreads) {
    const int row = find_row(ftab, n_rows, F_K, F_FOFF, f);
    const long* m = meta + (long)row * S_K;
    const double* p = prm + (long)row * P_K;
    const long n = m[S_N];
    const double x = tau[f], ts = p[P_TSTEP];
    auto t32 = [&](long j) { return (double)(float)((double)j * ts); };
    auto y32 = [&](long j) { return (double)(float)curve_at(m, p, curves, j); };
    double out;
    if (n == 1 || x >= t32(n - 1)) {
      out = y32(n - 1);
    } else {
      double q = floor(x / ts);
      long j = q < 0.0 ? 0 : (q > (double)(n - 2) ? n - 2 : (long)q);
      for (int it = 0; it < 4 && j > 0 && t32(j) > x; ++it) --j;
      for (int it = 0; it < 4 && j < n - 2 && t32(j + 1) <= x; ++it) ++j;
      const double x0 = t32(j), x1 = t32(j + 1), y0 = y32(j), y1 = y32(j + 1);
      if (x == x0) {
        out = y0;
      } else {
        const double slope = (y1 - y0) / (x1 - x0);
        out = slope * (x - x0) + y0;
      }
    }
    ref[f] = (float)out;
  }
}

// ---- dynamic metrics -----------------------------------------------------------------------------------------------
// out4[row] = {RMSE_cents, lag in frames, overshoot cents, final error cents} over the row's first L frames
__global__ __launch_bounds__(kThreads) void stim_metrics_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ ref,
                                                                const long* __restrict__ tracks,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_sum[kThreads];
  __shared__ long s_arg[kThreads];
  const int tid = threadIdx.x;
  const long* m = tracks + (long)blockIdx.x * M_K;
  const long L = m[M_N];
  const float* p = pred + m[M_POFF];
  const float* f = ref + m[M_ROFF];
  double* o = out + (long)blockIdx.x * 4;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (L <= 0) {
    if (tid < 4) o[tid] = nan;
    return;
  }
  // rms cents over the voiced reference frames (pe_pitch_metrics' expression), the two means, max(pred)
  double sq = 0.0, nv = 0.0, sp = 0.0, sr = 0.0, mx = -INFINITY;
  for (long i = tid; i < L; i += kThreads) {
    const float pv = p[i], fv = f[i];
    sp += (double)pv; sr += (double)fv;
    mx = fmax(mx, (double)pv);
    if (fv > 0.f) {
      nv += 1.0;
      const double d = 1200.0 * log2((double)fmaxf(pv, 1e-5f) / 55.0) - 1200.0 * log2((double)fv / 55.0);
      sq += d * d;
    }
  }
  sq = block_sum_d(sq, s_sum, tid); nv = block_sum_d(nv, s_sum, tid);
  const double mp = block_sum_d(sp, s_sum, tid) / (double)L, mr = block_sum_d(sr, s_sum, tid) / (double)L;
  const double peak = block_max_d(mx, s_sum, tid);
  // np.allclose(centred, 0): every |centred| <= 1e-8
  double fp = 0.0, fr = 0.0;
  for (long i = tid; i < L; i += kThreads) {
    fp = fmax(fp, fabs((double)p[i] - mp));
    fr = fmax(fr, fabs((double)f[i] - mr));
  }
  fp = block_max_d(fp, s_sum, tid); fr = block_max_d(fr, s_sum, tid);
  double lag = nan;
  if (fp > 1e-8 && fr > 1e-8) {
    // c[k] = sum over n of pred_c[n + k - (L - 1)] ref_c[n], k < 2 L - 1; the first maximum
    double best = -INFINITY;
    long arg = 2 * L;
    for (long k = tid; k < 2 * L - 1; k += kThreads) {
      const long sh = k - (L - 1);
      const long lo = sh < 0 ? -sh : 0, hi = sh > 0 ? L - sh : L;
      double c = 0.0;
      for (long i = lo; i < hi; ++i) c += ((double)p[i + sh] - mp) * ((double)f[i] - mr);
      if (c > best) { best = c; arg = k; }
    }
    s_sum[tid] = best; s_arg[tid] = arg;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
      if (tid < st) {
        const double b = s_sum[tid + st];
        const long a = s_arg[tid + st];
        if (b > s_sum[tid] || (b == s_sum[tid] && a < s_arg[tid])) { s_sum[tid] = b; s_arg[tid] = a; }
      }
      __syncthreads();
    }
    lag = (double)(s_arg[0] - (L - 1));
  }
  if (tid == 0) {
    const double target = (double)f[L - 1], last = (double)p[L - 1];
    o[0] = nv > 0 ? sqrt(sq / nv) : nan;
    o[1] = lag;
    o[2] = target > 0.0 && peak > 0.0 ? 1200.0 * log2(peak / target) : nan;
    o[3] = target > 0.0 ? 1200.0 * log2(fmax(last, 1e-5) / fmax(target, 1e-5)) : nan;
  }
}

}  // namespace

extern "C" int pe_stim_plan_fields(void) { return S_K; }
extern "C" int pe_stim_param_fields(void) { return P_K; }

/* Host-only layout and parameters; see include/pitchextractor_hip.h. */
extern "C" int pe_stim_plan(int n_rows, const long* n, const long* y_off, const int* kind, const double* raw6,
                            const double* partials, const int* n_partials, const long* curve_off,
                            const long* curve_len, const long* noise_off, double sr, long* consts4, long* meta,
                            double* params, long* totals2) {
  if (!consts4 || !totals2 || n_rows < 0 || n_rows > kMaxRows || !isfinite(sr) || !(sr > 0.0)) return PE_E_ARG;
  if (n_rows > 0 && (!n || !y_off || !kind || !raw6 || !partials || !n_partials || !curve_off || !curve_len ||
                     !noise_off || !meta || !params))
    return PE_E_ARG;
  const long fade = fade_samples(sr);
  consts4[0] = kPiece; consts4[1] = fade; consts4[2] = kMaxPartials; consts4[3] = ST_K;
  auto freq_ok = [](double v) { return isfinite(v) && v > 0.0; };
  long s = 0, pc = 0;
  for (int r = 0; r < n_rows; ++r) {
    const double* q = raw6 + 6L * r;                 // amplitude, a, b, c, duration, snr_db
    if (n[r] < 1 || n[r] > kMaxSamples || y_off[r] < 0 || kind[r] < 0 || kind[r] >= K_KINDS) return PE_E_ARG;
    if (fade > 0 && n[r] < fade) return PE_E_ARG;
    if (!isfinite(q[0]) || noise_off[r] < -1 || (noise_off[r] >= 0 && !isfinite(q[5]))) return PE_E_ARG;
    double* p = params + (long)r * P_K;
    for (int j = 0; j < P_K; ++j) p[j] = 0.0;
    long* m = meta + (long)r * S_K;
    int parts = 0;
    long coff = 0, clen = 0;
    p[P_AMP] = q[0]; p[P_SNR] = noise_off[r] >= 0 ? q[5] : 0.0; p[P_SR] = sr;
    if (kind[r] == K_CURVE) {
      if (curve_off[r] < 0 || (curve_len[r] != 1 && curve_len[r] != n[r])) return PE_E_ARG;
      if (!(isfinite(q[4]) && q[4] > 0.0)) return PE_E_ARG;
      coff = curve_off[r]; clen = curve_len[r];
    } else if (kind[r] == K_GLIDE) {
      if (!freq_ok(q[1]) || !freq_ok(q[2]) || !(isfinite(q[4]) && q[4] > 0.0)) return PE_E_ARG;
      p[P_A] = q[1]; p[P_C] = q[2];
      p[P_B] = n[r] > 1 ? (q[2] - q[1]) / (double)(n[r] - 1) : 0.0;
    } else if (kind[r] == K_VIBRATO) {               // a = base, b = depth in cents, c = rate
      if (!freq_ok(q[1]) || !isfinite(q[2]) || !isfinite(q[3]) || !(isfinite(q[4]) && q[4] > 0.0)) return PE_E_ARG;
      p[P_A] = q[1]; p[P_B] = q[2] / 1200.0; p[P_C] = kTwoPi * q[3];
    } else {
      if (!freq_ok(q[1]) || !(isfinite(q[4]) && q[4] > 0.0)) return PE_E_ARG;
      if (n_partials[r] < 1 || n_partials[r] > kMaxPartials) return PE_E_ARG;
      parts = n_partials[r];
      p[P_A] = q[1];
      for (int h = 0; h < parts; ++h) {               // {harmonic, amplitude}
        const double hn = partials[(2L * kMaxPartials) * r + 2 * h], ha = partials[(2L * kMaxPartials) * r + 2 * h + 1];
        if (!isfinite(hn) || !isfinite(ha)) return PE_E_ARG;
        p[P_PARTIALS + 2 * h] = ha;
        p[P_PARTIALS + 2 * h + 1] = (kTwoPi * q[1]) * hn;
      }
    }
    p[P_TSTEP] = q[4] / (double)n[r];
    m[S_OFF] = y_off[r]; m[S_N] = n[r]; m[S_KIND] = kind[r]; m[S_SOFF] = s;
    m[S_PIECES] = (n[r] + kPiece - 1) / kPiece; m[S_POFF] = pc; m[S_COFF] = coff; m[S_CLEN] = clen;
    m[S_NPART] = parts; m[S_FADE] = fade; m[S_NOFF] = noise_off[r];
    s += n[r]; pc += m[S_PIECES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_PIECES] = pc;
  return PE_OK;
}

extern "C" size_t pe_stim_workspace_bytes(long pieces) {
  return pieces > 0 ? (size_t)pieces * 3 * sizeof(double) : 0;
}

namespace {
bool has_curve_rows(const long* hm, int n_rows) {
  for (int r = 0; r < n_rows; ++r)
    if (hm[(long)r * S_K + S_KIND] == K_CURVE) return true;
  return false;
}
bool has_noise_rows(const long* hm, int n_rows) {
  for (int r = 0; r < n_rows; ++r)
    if (hm[(long)r * S_K + S_NOFF] >= 0) return true;
  return false;
}
}  // namespace

extern "C" int pe_stim_phase(const long* meta, const long* host_meta, const double* params, const float* curves,
                             int n_rows, double* phase, void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!meta || !params || !phase || (has_curve_rows(host_meta, n_rows) && !curves)) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_stim_workspace_bytes(tot[TOT_PIECES])) return PE_E_WORKSPACE;
  double* sums = static_cast<double*>(workspace);
  const long pieces = tot[TOT_PIECES];
  const dim3 grid(grid_of(pieces)), wg(kThreads);
  hipLaunchKernelGGL(stim_phase_kernel<false>, grid, wg, 0, pe_stream(stream), meta, params, curves, n_rows, pieces,
                     sums, phase);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(stim_carry_kernel, dim3((n_rows + kThreads - 1) / kThreads), wg, 0, pe_stream(stream), meta,
                     n_rows, sums);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(stim_phase_kernel<true>, grid, wg, 0, pe_stream(stream), meta, params, curves, n_rows, pieces,
                     sums, phase);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stim_synth(const long* meta, const long* host_meta, const double* params, const double* phase,
                             int n_rows, float* y, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!meta || !params || !phase || !y) return PE_E_ARG;
  hipLaunchKernelGGL(stim_synth_kernel, dim3(grid_of(tot[TOT_PIECES])), dim3(kThreads), 0, pe_stream(stream), meta,
                     params, phase, n_rows, tot[TOT_PIECES], y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stim_tone(const long* meta, const long* host_meta, const double* params, int n_rows, float* y,
                            void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!meta || !params || !y) return PE_E_ARG;
  hipLaunchKernelGGL(stim_tone_kernel, dim3(grid_of(tot[TOT_PIECES])), dim3(kThreads), 0, pe_stream(stream), meta,
                     params, n_rows, tot[TOT_PIECES], y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_stim_finish(const long* meta, const long* host_meta, const double* params, const float* noise,
                              int n_rows, float* y, double* stats, void* workspace, size_t workspace_bytes,
                              void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!meta || !params || !y || !stats || (has_noise_rows(host_meta, n_rows) && !noise)) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_stim_workspace_bytes(tot[TOT_PIECES])) return PE_E_WORKSPACE;
  return launch_snr_mix<StimMixRows>(meta, n_rows, params + P_SNR, tot[TOT_PIECES], y, noise, y, true, stats,
                                     static_cast<double*>(workspace), pe_stream(stream));
}

extern "C" int pe_stim_reference(const long* meta, const long* host_meta, const double* params, const float* curves,
                                 const long* frame_table, const long* host_frame_table, const double* frame_times,
                                 int n_rows, float* ref, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!host_frame_table) return PE_E_ARG;
  long frames = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* ft = host_frame_table + (long)r * F_K;
    if (ft[F_NF] < 0 || ft[F_FOFF] != frames) return PE_E_ARG;
    frames += ft[F_NF];
  }
  if (frames == 0) return PE_OK;
  if (!meta || !params || !frame_table || !frame_times || !ref || (has_curve_rows(host_meta, n_rows) && !curves))
    return PE_E_ARG;
  hipLaunchKernelGGL(stim_reference_kernel, dim3(grid_for(frames, kThreads, 1 << 16)), dim3(kThreads), 0,
                     pe_stream(stream), meta, params, curves, frame_table, frame_times, n_rows, frames, ref);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_dynamic_metrics_fields(void) { return M_K; }

extern "C" int pe_dynamic_metrics(const float* f0_pred, const float* f0_ref, const long* tracks,
                                  const long* host_tracks, int n_rows, double* out4, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows == 0) return PE_OK;
  if (!host_tracks) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = host_tracks + (long)r * M_K;
    if (m[M_POFF] < 0 || m[M_N] < 0 || m[M_N] > (1L << 30) || m[M_ROFF] < 0) return PE_E_ARG;
  }
  if (!f0_pred || !f0_ref || !tracks || !out4) return PE_E_ARG;
  hipLaunchKernelGGL(stim_metrics_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), f0_pred, f0_ref, tracks,
                     out4);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
