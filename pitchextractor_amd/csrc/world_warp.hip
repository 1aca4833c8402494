// Voice transforms in the WORLD domain: a row's spectral envelopes (CheapTrick's layout) and aperiodicities read at
// other frame positions (tempo), along a warped frequency axis (vocal-tract length: the piecewise-linear map of Jaitly &
// Hinton, "Vocal Tract Length Perturbation improves speech recognition", 2013), tilted, and with the aperiodicity scaled
// (breath).  pe_world_warp_plan (host only) lays the batch out in the frame plan of world_frames.h with three fields of
// its own; pe_world_warp is one launch with one workgroup per (row, output frame).
//
// Per output frame: its source position is an integer frame fi and a fraction in [0, 1) (the host forms both in
// float64).  The workgroup stages, once per source bin, ln sp[fi] + frac (ln sp[fi + 1] - ln sp[fi]) in LDS (and the
// same mix of ap in the linear domain), so a source bin costs one log per source frame and output frame; fi + 1 is
// clamped to the row's last frame, and a fraction of 0 reads one frame only.  Output bin k then reads the staged row at
// u = w^-1(k) bins, linearly between floor(u) and floor(u) + 1, where w(f) = alpha f up to f_hi min(alpha, 1) / alpha
// and from there the straight line to (fs / 2, fs / 2); adds tilt_db_per_octave log2(max(f, 125) / 1000) dB and takes
// one exp.  ap: the same read, times 10^(breath_db / 20), clamped to [0, 1].
//
// Identity is a copy: alpha == 1, no tilt and a fraction of 0 copy the source frame's sp bit for bit, and its ap when
// breath_db == 0 as well; the branch depends on the row's record and the frame's position only, so it is
// workgroup-uniform.  float32 per bin (the map's four per-row constants are formed in double), no scratch, no atomics,
// no traffic between workgroups, every output element written once: a row is bit-identical alone, at any offset,
// padded, anywhere in a batch and into a wider stride.  Rows are read and written one float per lane, consecutive
// lanes on consecutive bins: the offsets are arbitrary, so there is no wider aligned access to be had.
#include <math.h>
#include <vector>
#include "common.h"
#include "world_frames.h"

using namespace pe;

namespace {

constexpr int kThreads = kFrameThreads;
constexpr int kMaxBins = 2048 / 2 + 1;
constexpr int kParams = 4;                                       // {alpha, f_hi, tilt dB / octave, breath dB} per row
enum { P_ALPHA, P_FHI, P_TILT, P_BREATH };
// The frame plan's fields stand for: FR_XOFF the row's frame 0 in sp_in, FR_N its source frames, FR_F0OFF = FR_FOFF
// its first output frame in the position arrays, FR_FIRST 0, FR_FRAMES its output frames, FR_OOFF / FR_OSTRIDE where
// output frame q goes.  Then the plan's own:
enum { WP_ISTRIDE = FR_K, WP_AOFF, WP_ASTRIDE, WP_K };         // source stride; the row's frame 0 in ap_in (< 0: none)

int config_status(double fs, int fft_size) {
  if (!(fs > 0.0) || !isfinite(fs)) return PE_E_ARG;
  return world_fft_size_ok(fft_size) ? PE_OK : PE_E_UNSUPPORTED;
}

// the walk over the plan's host copy that the launch relies on; fills {output frames} and whether a row has an ap
bool warp_plan_consistent(const long* hm, int n_rows, int fft_size, long* frames, bool* any_ap) {
  if (!frame_plan_consistent(hm, n_rows, fft_size, frames, WP_K)) return false;
  *any_ap = false;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * WP_K;
    if (m[FR_FIRST] != 0 || m[FR_F0OFF] != m[FR_FOFF] || m[WP_ISTRIDE] < 0 || m[WP_ASTRIDE] < 0) return false;
    *any_ap = *any_ap || m[WP_AOFF] >= 0;
  }
  return true;
}

// The inverse map in bins: u(k) = k inv_alpha for k <= y0, else x0 + (k - y0) slope.
struct InverseMap {
  float inv_alpha, y0, x0, slope;
};

__device__ __forceinline__ InverseMap inverse_map(float alpha, float f_hi, double fs, int fft_size) {
  const double a = (double)alpha, per_bin = fs / (double)fft_size, half = 0.5 * (double)fft_size;
  const double x0 = (double)f_hi * (a < 1.0 ? a : 1.0) / a / per_bin, y0 = a * x0;
  InverseMap m;
  m.inv_alpha = (float)(1.0 / a);
  m.y0 = (float)y0;
  m.x0 = (float)x0;
  m.slope = (float)((half - x0) / (half - y0));
  return m;
}

// src[u] between the two bins around u, for a row of H + 1 staged values
__device__ __forceinline__ float read_at(const float* s, const InverseMap& im, int k, int H) {
  const float kf = (float)k;
  const float u = kf <= im.y0 ? kf * im.inv_alpha : im.x0 + (kf - im.y0) * im.slope;
  int k0 = (int)floorf(u);
  k0 = k0 < 0 ? 0 : (k0 > H - 1 ? H - 1 : k0);
  float t = u - (float)k0;
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  const float a = s[k0], b = s[k0 + 1];
  return a + t * (b - a);
}

__global__ __launch_bounds__(kThreads) void world_warp_kernel(const float* __restrict__ sp_in,
                                                              const float* __restrict__ ap_in,
                                                              const long* __restrict__ meta,
                                                              const int* __restrict__ pos_frame,
                                                              const float* __restrict__ pos_frac,
                                                              const float* __restrict__ params, int n_rows,
                                                              long n_frames, double fs, int fft_size,
                                                              float* __restrict__ sp_out, float* __restrict__ ap_out) {
  __shared__ float s_sp[kMaxBins];
  __shared__ float s_ap[kMaxBins];
  const int tid = threadIdx.x, H = fft_size / 2, bins = H + 1;
  const float hz_per_bin = (float)(fs / (double)fft_size);
  for (long g = blockIdx.x; g < n_frames; g += gridDim.x) {
    const int row = find_row(meta, n_rows, WP_K, FR_FOFF, g);
    const long* m = meta + (long)row * WP_K;
    const long src = m[FR_N], q = g - m[FR_FOFF];
    long fi = pos_frame[g];
    fi = fi < 0 ? 0 : (fi > src - 1 ? src - 1 : fi);              // the plan has checked the positions: memory safety
    const long fj = fi + 1 < src ? fi + 1 : src - 1;
    const float frac = fj == fi ? 0.f : pos_frac[g];
    const float* p = params + (long)row * kParams;
    const float alpha = p[P_ALPHA], tilt = p[P_TILT], breath = p[P_BREATH];
    const bool same_axes = alpha == 1.f && tilt == 0.f && frac == 0.f;        // uniform over the workgroup
    const InverseMap im = inverse_map(alpha, p[P_FHI], fs, fft_size);
    const float* a0 = sp_in + m[FR_XOFF] + fi * m[WP_ISTRIDE];
    const float* a1 = sp_in + m[FR_XOFF] + fj * m[WP_ISTRIDE];
    float* o = sp_out + m[FR_OOFF] + q * m[FR_OSTRIDE];
    const bool has_ap = m[WP_AOFF] >= 0;
    const bool stage_ap = has_ap && !(same_axes && breath == 0.f);
    const float* b0 = ap_in + (has_ap ? m[WP_AOFF] + fi * m[WP_ASTRIDE] : 0);
    const float* b1 = ap_in + (has_ap ? m[WP_AOFF] + fj * m[WP_ASTRIDE] : 0);
    float* oa = ap_out + (has_ap ? m[FR_OOFF] + q * m[FR_OSTRIDE] : 0);
    if (same_axes) {
      for (int k = tid; k < bins; k += kThreads) o[k] = a0[k];
    } else {
      for (int k = tid; k < bins; k += kThreads) {
        float l = logf(a0[k]);
        if (frac != 0.f) l += frac * (logf(a1[k]) - l);
        s_sp[k] = l;
      }
    }
    if (has_ap && !stage_ap) {
      for (int k = tid; k < bins; k += kThreads) oa[k] = b0[k];
    } else if (stage_ap) {
      for (int k = tid; k < bins; k += kThreads) {
        float v = b0[k];
        if (frac != 0.f) v += frac * (b1[k] - v);
        s_ap[k] = v;
      }
    }
    __syncthreads();
    if (!same_axes) {
      const float ln_per_db = 0.23025850929940457f;               // ln(10) / 10: sp is a power
      for (int k = tid; k < bins; k += kThreads) {
        float v = read_at(s_sp, im, k, H);
        if (tilt != 0.f) v += tilt * log2f(fmaxf((float)k * hz_per_bin, 125.f) / 1000.f) * ln_per_db;
        o[k] = expf(v);
      }
    }
    if (stage_ap) {
      const float gain = exp10f(breath / 20.f);
      for (int k = tid; k < bins; k += kThreads) oa[k] = fminf(fmaxf(read_at(s_ap, im, k, H) * gain, 0.f), 1.f);
    }
    __syncthreads();                                             // the next frame's staging overwrites the rows
  }
}

}  // namespace

extern "C" int pe_world_warp_plan_fields(void) { return WP_K; }

/* Host-only batch layout; see include/pitchextractor_hip.h. */
extern "C" int pe_world_warp_plan(int n_rows, const long* src_frames, const long* in_off, const long* in_stride,
                                  const long* ap_off, const long* ap_stride, const long* out_frames,
                                  const long* out_off, const long* out_stride, const int* pos_frame,
                                  const float* pos_frac, const float* params, double fs, int fft_size, long* meta,
                                  long* totals) {
  if (n_rows < 0 || n_rows > kMaxRows || !totals) return PE_E_ARG;
  int st = config_status(fs, fft_size);
  if (st != PE_OK) return st;
  if (n_rows > 0 && (!src_frames || !in_off || !in_stride || !out_frames || !out_off || !out_stride || !params ||
                     !meta || (ap_off && !ap_stride)))
    return PE_E_ARG;
  // the frame plan with: f0_off = the row's first output frame in the position arrays, f0_len = its output frames
  std::vector<long> pos_off(n_rows), zero(n_rows, 0);
  long tot = 0;
  for (int r = 0; r < n_rows; ++r) {
    if (out_frames[r] < 0) return PE_E_ARG;
    pos_off[r] = tot;
    tot += out_frames[r];
  }
  if ((st = frame_plan_fill(n_rows, in_off, src_frames, pos_off.data(), out_frames, zero.data(), out_frames, out_off,
                            out_stride, fft_size, meta, totals, WP_K)) != PE_OK)
    return st;
  if (tot > 0 && (!pos_frame || !pos_frac)) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    const bool has_ap = ap_off && ap_off[r] >= 0;
    if (in_stride[r] < 0 || (has_ap && ap_stride[r] < 0)) return PE_E_ARG;
    const float* p = params + (long)r * kParams;
    if (!isfinite(p[P_ALPHA]) || p[P_ALPHA] < 0.5f || p[P_ALPHA] > 2.f || !isfinite(p[P_TILT]) ||
        !isfinite(p[P_BREATH]))
      return PE_E_ARG;
    // w rises strictly from (0, 0) to the knee and on to (fs / 2, fs / 2) exactly when the knee lies inside
    if (!isfinite(p[P_FHI]) || !(p[P_FHI] > 0.f) || !((double)p[P_FHI] < 0.5 * fs)) return PE_E_ARG;
    for (long q = 0; q < out_frames[r]; ++q) {
      const long f = pos_frame[pos_off[r] + q];
      const float t = pos_frac[pos_off[r] + q];
      if (f < 0 || !(t >= 0.f) || !(t < 1.f) || f > src_frames[r] - 1 || (f == src_frames[r] - 1 && t != 0.f))
        return PE_E_ARG;
    }
    long* m = meta + (long)r * WP_K;
    m[WP_ISTRIDE] = in_stride[r];
    m[WP_AOFF] = has_ap ? ap_off[r] : -1;
    m[WP_ASTRIDE] = has_ap ? ap_stride[r] : 0;
  }
  return PE_OK;
}

extern "C" int pe_world_warp(const float* sp_in, const float* ap_in, const long* meta, const long* host_meta,
                             const int* pos_frame, const float* pos_frac, const float* params, int n_rows, double fs,
                             int fft_size, float* sp_out, float* ap_out, void* stream) {
  long frames = 0;
  bool any_ap = false;
  PE_OPEN(open_rows(n_rows, config_status(fs, fft_size), host_meta,
                    [&] { return warp_plan_consistent(host_meta, n_rows, fft_size, &frames, &any_ap); }, &frames));
  if (!sp_in || !meta || !pos_frame || !pos_frac || !params || !sp_out || (any_ap && (!ap_in || !ap_out)))
    return PE_E_ARG;
  hipLaunchKernelGGL(world_warp_kernel, dim3(grid_for(frames, 1, 65536)), dim3(kThreads), 0, pe_stream(stream), sp_in,
                     ap_in, meta, pos_frame, pos_frac, params, n_rows, frames, fs, fft_size, sp_out, ap_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
