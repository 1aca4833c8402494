// Pitch modulation of real audio on ragged batches: a time warp y(t) = x(tau(t)) over the span a row's kept label
// frames cover, read through a band-limited interpolator whose position and cutoff change per sample, and the label
// pass that moves f0 and the silence flags with it.  Pinned by the float64 restatement in tests/pitch_mod_ref.py.
//
// The time map is closed form, in double, a pure function of the row's parameters and u = t - t0 (no running sum, so
// nothing depends on where a row or a tile lies): up to 4 sinusoids (d_k, w_k = 2 pi rate_k / sr, phi_k) and a ramp a,
//   m(u)   = sum_k d_k sin(w_k u + phi_k) + a (2u/T - 1)
//   mbar   = (1/T) sum_k d_k (cos phi_k - cos(w_k T + phi_k)) / w_k
//   s(u)   = 1 + m(u) - mbar                                          the local speed: every harmonic is multiplied by it
//   tau(u) = u (1 - mbar) + a (u^2/T - u) + sum_k d_k (cos phi_k - cos(w_k u + phi_k)) / w_k
// with tau = u exactly at u = 0 and u = T (both ends pinned), the identity outside [t0, t1].  The plan refuses
// 2 sum|d_k| + |a| > 0.5, which keeps s within [0.5, 1.5] and tau monotone.
//
// pm_wave_kernel: one workgroup per (row, tile of kTile consecutive output samples).  Output sample i in (t0, t1) reads
// p = t0 + tau(i - t0) with scale = min(1, 1 / s):  y[i] = scale * sum_s W(scale |p - s|) x[s], W the piecewise-linear
// read (value + eta * difference, 512 entries per zero crossing) of the resampy-style filter that ps_resample_kernel
// reads, here with the scale per sample and the table position (frac + a) scale 512 formed per tap in double instead
// of advanced by a truncated integer step.  Taps in a fixed order (the left wing from floor(p) down, then the right
// wing up), float32 accumulation.  tau is monotone, so a tile's sources are contiguous: at most 1.5 kTile samples plus
// two wings of 24 / 96; they are staged in LDS once per workgroup (a read that falls outside the staged span, which
// the plan's cap excludes, goes to memory under the row's bounds: staging is never what keeps an index in range).
// The filter table, interleaved {value, difference}, is read from L2 or, for kaiser_fast (64 KiB), from a copy each
// workgroup makes in LDS; the caller picks, the bits are the same.  Samples outside the span, rows not selected and
// identity modulations are copied bit for bit; every element of [0, n) is written once, out of place, no atomics.
//
// pm_labels_kernel: one thread per (row, kept frame j): pos = tau(j hop) / hop, read by world.time_warp_curve's rule
// (linear between two voiced frames; across a voicing boundary the nearer frame, the earlier on a tie), a voiced
// result multiplied by s.
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 2048;                                  // output samples of one workgroup
constexpr int kP = 512;                                      // table entries per zero crossing (resampy's 2^9)
constexpr int kZeros[2] = {64, 16};                          // kaiser_best, kaiser_fast (pitch_shift.hip's order)
constexpr int kWingMax = 96;                                 // 1.5 x 64 zero crossings at scale = 1 / 1.5
constexpr int kSpan = kTile * 3 / 2 + 2 * kWingMax + 8;      // staged source samples: 13 KB
constexpr int kMaxSin = 4;
constexpr double kCap = 0.5;                                 // 2 sum|d_k| + |a| <= kCap
constexpr double kMinRate = 0.05;                            // Hz
constexpr long kMaxSamples = (1L << 31) - 8;

// per-row parameters (double)
enum { P_D = 0, P_W = 4, P_PHI = 8, P_COSPHI = 12, P_A = 16, P_MBAR = 17, P_T = 18, P_K = 24 };
// the caller's modulation row: d[4], rate_hz[4], phi[4], a
enum { G_D = 0, G_RATE = 4, G_PHI = 8, G_A = 12, G_K = 13 };
// per-row plan fields (int64)
enum { M_XOFF, M_N, M_YOFF, M_T0, M_T1, M_ON, M_FRAMES, M_TOFF, M_K };
static_assert(M_XOFF == kRowOffset && M_N == kRowLength, "every row plan opens with offset and length");

// (tau, s) at u in [0, T] from a row's parameters
__device__ __forceinline__ void time_map(const double* P, double u, double& tau, double& s) {
  const double T = P[P_T], a = P[P_A], mbar = P[P_MBAR];
  double m = 0.0, c = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxSin; ++k) {
    const double d = P[P_D + k];
    if (d != 0.0) {
      const double w = P[P_W + k];
      double sn, cs;
      sincos(w * u + P[P_PHI + k], &sn, &cs);
      m += d * sn;
      c += d * (P[P_COSPHI + k] - cs) / w;
    }
  }
  s = 1.0 + m + a * (2.0 * u / T - 1.0) - mbar;
  tau = u * (1.0 - mbar) + a * (u * u / T - u) + c;
  if (u <= 0.0) tau = 0.0;
  if (u >= T) tau = T;
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void pm_wave_kernel(const float* __restrict__ x, const long* __restrict__ meta,
                                                           const double* __restrict__ params, int n_rows,
                                                           const float2* __restrict__ table, int nwin, int wing,
                                                           float* __restrict__ y) {
  extern __shared__ float2 s_tab[];                          // nwin pairs when LDS_TABLE
  __shared__ float s_x[kSpan];
  __shared__ double s_p[P_K];
  __shared__ long s_ends[2];
  const int tid = threadIdx.x;
  const long g = blockIdx.x;
  const int row = find_row(meta, n_rows, M_K, M_TOFF, g);
  const long* m = meta + (long)row * M_K;
  const long n = m[M_N], t0 = m[M_T0], t1 = m[M_T1];
  const long i0 = (g - m[M_TOFF]) * kTile;
  const long i1 = n < i0 + kTile ? n : i0 + kTile;
  const float* xr = x + m[M_XOFF];
  float* yr = y + m[M_YOFF];
  const long wa = i0 > t0 + 1 ? i0 : t0 + 1, wb = i1 < t1 ? i1 : t1;      // the tile's warped samples [wa, wb)
  if (m[M_ON] == 0 || wa >= wb) {                            // uniform over the workgroup
    for (long i = i0 + tid; i < i1; i += kThreads) yr[i] = xr[i];
    return;
  }
  if (tid < P_K) s_p[tid] = params[(long)row * P_K + tid];
  if constexpr (LDS_TABLE)
    for (int j = tid; j < nwin; j += kThreads) s_tab[j] = table[j];
  __syncthreads();
  if (tid < 2) {
    double tau, s;
    time_map(s_p, (double)((tid == 0 ? wa : wb - 1) - t0), tau, s);
    s_ends[tid] = t0 + (long)floor(tau);
  }
  __syncthreads();
  const long lo = s_ends[0] - wing;
  long len = s_ends[1] + wing + 2 - lo;
  len = len < 0 ? 0 : (len > kSpan ? kSpan : len);
  for (int j = tid; j < (int)len; j += kThreads) {
    const long s = lo + j;
    s_x[j] = (s >= 0 && s < n) ? xr[s] : 0.f;
  }
  __syncthreads();
  const float2* tab = table;
  if constexpr (LDS_TABLE) tab = s_tab;
  const double top = (double)(nwin - 1);
  auto source = [&](long s) -> float {
    const long j = s - lo;
    if (j >= 0 && j < len) return s_x[j];
    return (s >= 0 && s < n) ? xr[s] : 0.f;
  };
  for (long i = i0 + tid; i < i1; i += kThreads) {
    float out;
    if (i <= t0 || i >= t1) {
      out = xr[i];
    } else {
      double tau, s;
      time_map(s_p, (double)(i - t0), tau, s);
      const double p = (double)t0 + tau;
      const double scale = s > 1.0 ? 1.0 / s : 1.0;
      const double sp = scale * kP;
      const double fl = floor(p);
      const long n0 = (long)fl;
      const double frac = p - fl;
      float v = 0.f;
      for (int a = 0; a <= kWingMax; ++a) {                  // the left wing: floor(p) and down
        const double xt = (frac + (double)a) * sp;
        if (!(xt < top)) break;
        const int off = (int)xt;
        const float eta = (float)(xt - (double)off);
        const float2 wd = tab[off];
        v = fmaf(fmaf(eta, wd.y, wd.x), source(n0 - a), v);
      }
      for (int a = 0; a <= kWingMax; ++a) {                  // the right wing: floor(p) + 1 and up
        const double xt = ((1.0 - frac) + (double)a) * sp;
        if (!(xt < top)) break;
        const int off = (int)xt;
        const float eta = (float)(xt - (double)off);
        const float2 wd = tab[off];
        v = fmaf(fmaf(eta, wd.y, wd.x), source(n0 + 1 + a), v);
      }
      out = v * (float)scale;
    }
    yr[i] = out;
  }
}

__global__ __launch_bounds__(kThreads) void pm_labels_kernel(const float* __restrict__ f0, const float* __restrict__ sil,
                                                             const long* __restrict__ meta,
                                                             const double* __restrict__ params, int n_rows, int hop,
                                                             int width, float* __restrict__ f0_out,
                                                             float* __restrict__ sil_out) {
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= (long)n_rows * width) return;
  const int row = (int)(g / width), j = (int)(g % width);
  const long* m = meta + (long)row * M_K;
  const float* fr = f0 + (long)row * width;
  const float* qr = sil + (long)row * width;
  const long L = m[M_FRAMES];
  float f = fr[j], q = qr[j];
  if (m[M_ON] != 0 && j < L) {
    const double* P = params + (long)row * P_K;
    double tau, s;
    time_map(P, (double)j * (double)hop, tau, s);
    const double pos = tau / (double)hop;
    long i = (long)floor(pos);
    i = i < 0 ? 0 : (i > L - 1 ? L - 1 : i);
    const long k = i + 1 < L - 1 ? i + 1 : L - 1;
    double t = pos - (double)i;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const float a = fr[i], b = fr[k];
    const bool va = a > 0.f && qr[i] == 0.f, vb = b > 0.f && qr[k] == 0.f;
    if (va && vb) {
      f = (float)(s * ((double)a + t * ((double)b - (double)a)));
      q = 0.f;
    } else {
      const long pick = t <= 0.5 ? i : k;
      const bool voiced = t <= 0.5 ? va : vb;
      f = voiced ? (float)(s * (double)fr[pick]) : fr[pick];
      q = voiced ? 0.f : qr[pick];
    }
  }
  f0_out[g] = f;
  sil_out[g] = q;
}

// a row's modulation {d[4], rate_hz[4], phi[4], a}: 0 = the identity, 1 = within the limits, -1 = refused
int mod_class(const double* G) {
  double sum = 0.0;
  bool any = false;
  for (int j = 0; j < G_K; ++j)
    if (!isfinite(G[j])) return -1;
  for (int k = 0; k < kMaxSin; ++k) {
    if (G[G_D + k] == 0.0) continue;
    if (!(G[G_RATE + k] >= kMinRate)) return -1;
    sum += fabs(G[G_D + k]);
    any = true;
  }
  if (G[G_A] != 0.0) any = true;
  if (!(2.0 * sum + fabs(G[G_A]) <= kCap)) return -1;
  return any ? 1 : 0;
}

// the plan's host copy and its parameters as pe_pitch_mod_plan makes them
bool rows_ok(const long* host_meta, const double* host_params, int n_rows, long* tiles, long* warped) {
  long t = 0;
  *warped = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = host_meta + (long)r * M_K;
    if (m[M_XOFF] < 0 || m[M_YOFF] < 0 || m[M_N] < 0 || m[M_N] > kMaxSamples || m[M_TOFF] != t) return false;
    if (m[M_ON] != 0) {
      if (!host_params || m[M_ON] != 1 || m[M_T0] < 0 || m[M_T1] <= m[M_T0] || m[M_T1] > m[M_N] || m[M_FRAMES] < 2)
        return false;
      const double* P = host_params + (long)r * P_K;
      double sum = 0.0;
      for (int j = 0; j < P_K; ++j)
        if (!isfinite(P[j])) return false;
      for (int k = 0; k < kMaxSin; ++k) {
        if (P[P_D + k] != 0.0 && !(P[P_W + k] > 0.0)) return false;
        sum += fabs(P[P_D + k]);
      }
      if (!(2.0 * sum + fabs(P[P_A]) <= kCap) || P[P_T] != (double)(m[M_T1] - m[M_T0])) return false;
      ++*warped;
    }
    t += (m[M_N] + kTile - 1) / kTile;
  }
  *tiles = t;
  return true;
}

}  // namespace

/* Host only; see include/pitchextractor_hip.h. */
extern "C" int pe_pitch_mod_consts(long* consts4) {
  if (!consts4) return PE_E_ARG;
  consts4[0] = kTile; consts4[1] = kThreads; consts4[2] = kSpan; consts4[3] = kMaxSin;
  return PE_OK;
}

extern "C" int pe_pitch_mod_plan_fields(void) { return M_K; }

extern "C" int pe_pitch_mod_plan(int n_rows, const long* n, const long* x_off, const long* y_off, const long* t0,
                                 const long* t1, const int* on, const double* mods, int sr, int hop, long* meta,
                                 double* params, long* totals2) {
  if (n_rows < 0 || n_rows > kMaxRows || sr <= 0 || hop <= 0 || !totals2) return PE_E_ARG;
  if (n_rows > 0 && (!n || !x_off || !y_off || !t0 || !t1 || !on || !mods || !meta || !params)) return PE_E_ARG;
  long tiles = 0, warped = 0;
  for (int r = 0; r < n_rows; ++r) {
    if (n[r] < 0 || n[r] > kMaxSamples || x_off[r] < 0 || y_off[r] < 0) return PE_E_ARG;
    long* m = meta + (long)r * M_K;
    double* P = params + (long)r * P_K;
    for (int j = 0; j < P_K; ++j) P[j] = 0.0;
    int cls = 0;
    if (on[r]) {
      const double* G = mods + (long)r * G_K;
      cls = mod_class(G);
      if (cls < 0) return PE_E_ARG;
      const long span = t1[r] - t0[r];
      if (t0[r] < 0 || t1[r] > n[r] || span < hop || span % hop != 0) return PE_E_ARG;
      if (cls > 0) {
        const double T = (double)span;
        double mbar = 0.0;
        for (int k = 0; k < kMaxSin; ++k) {
          const double d = G[G_D + k];
          if (d == 0.0) continue;
          const double w = 2.0 * M_PI * G[G_RATE + k] / (double)sr, phi = G[G_PHI + k];
          P[P_D + k] = d; P[P_W + k] = w; P[P_PHI + k] = phi; P[P_COSPHI + k] = cos(phi);
          mbar += d * (cos(phi) - cos(w * T + phi)) / w;
        }
        P[P_A] = G[G_A]; P[P_MBAR] = mbar / T; P[P_T] = T;
      }
    }
    m[M_XOFF] = x_off[r]; m[M_N] = n[r]; m[M_YOFF] = y_off[r]; m[M_T0] = t0[r]; m[M_T1] = t1[r];
    m[M_ON] = cls > 0 ? 1 : 0;
    m[M_FRAMES] = cls > 0 ? (t1[r] - t0[r]) / hop + 1 : 0;
    m[M_TOFF] = tiles;
    tiles += (n[r] + kTile - 1) / kTile;
    warped += cls > 0 ? 1 : 0;
  }
  totals2[0] = tiles; totals2[1] = warped;
  return PE_OK;
}

extern "C" int pe_pitch_mod_wave(const float* x, const long* meta, const long* host_meta, const double* params,
                                 const double* host_params, int n_rows, const float* table, int res_type,
                                 int table_in_lds, float* y, void* stream) {
  if (res_type < 0 || res_type > 1 || table_in_lds < 0 || table_in_lds > 1) return PE_E_ARG;
  if (table_in_lds && kZeros[res_type] != 16) return PE_E_UNSUPPORTED;      // kaiser_best is 256 KiB
  long tiles = 0, warped = 0;
  PE_OPEN(open_rows(n_rows, PE_OK, host_meta, [&] { return rows_ok(host_meta, host_params, n_rows, &tiles, &warped); },
                    &tiles));
  if (!x || !meta || !params || !table || !y || x == y || tiles > (1L << 30)) return PE_E_ARG;
  const int nwin = kZeros[res_type] * kP + 1, wing = kZeros[res_type] * 3 / 2;
  const float2* tab = reinterpret_cast<const float2*>(table);
  if (table_in_lds) {
    const size_t bytes = (size_t)nwin * sizeof(float2);
    PE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_wave_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(pm_wave_kernel<true>, dim3((unsigned)tiles), dim3(kThreads), bytes, pe_stream(stream), x, meta,
                       params, n_rows, tab, nwin, wing, y);
  } else {
    hipLaunchKernelGGL(pm_wave_kernel<false>, dim3((unsigned)tiles), dim3(kThreads), 0, pe_stream(stream), x, meta,
                       params, n_rows, tab, nwin, wing, y);
  }
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_pitch_mod_labels(const float* f0, const float* sil, const long* meta, const long* host_meta,
                                   const double* params, const double* host_params, int n_rows, int hop, int width,
                                   float* f0_out, float* sil_out, void* stream) {
  if (hop <= 0 || width < 0) return PE_E_ARG;
  long tiles = 0, warped = 0;
  const long work = (long)(n_rows > 0 ? n_rows : 0) * width;
  PE_OPEN(open_rows(n_rows, PE_OK, host_meta, [&] { return rows_ok(host_meta, host_params, n_rows, &tiles, &warped); },
                    &work));
  for (int r = 0; r < n_rows; ++r) {
    const long* m = host_meta + (long)r * M_K;
    if (m[M_ON] != 0 && (m[M_FRAMES] > width || m[M_T1] - m[M_T0] != (m[M_FRAMES] - 1) * (long)hop)) return PE_E_ARG;
  }
  if (!f0 || !sil || !meta || !params || !f0_out || !sil_out || f0 == f0_out || sil == sil_out) return PE_E_ARG;
  hipLaunchKernelGGL(pm_labels_kernel, dim3(grid_of((work + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     pe_stream(stream), f0, sil, meta, params, n_rows, hop, width, f0_out, sil_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
