// Polyphase sinc resampler on the GPU: the arithmetic of
// torchaudio.functional.resample(x, orig, new) with its defaults -- sinc_interp_hann,
// lowpass_filter_width = 6, rolloff = 0.99 -- as the reference calls it at meldataset.py:621-627
// (44 100 -> 24 000 Hz reduces to 147 -> 80: 80 phases x 171 taps, output length ceil(80 L / 147)).
// One thread per output sample; the 54 KB tap table stays in L1/L2.
#include <math.h>
#include <vector>
#include "common.h"

struct pe_resample_plan {
  int orig, neu, width, taps;
  float* d_kernel;          // [neu][taps]
};

namespace {

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, long x_stride, int n_in,
                                                       float* __restrict__ y, long y_stride, int n_out,
                                                       const float* __restrict__ k, int orig, int neu, int width,
                                                       int taps) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= n_out) return;
  const float* xb = x + (long)blockIdx.y * x_stride;
  const int j = n / neu, p = n - j * neu;
  const float* kp = k + (long)p * taps;
  const int base = j * orig - width;
  float acc = 0.f;
  for (int i = 0; i < taps; ++i) {
    const int q = base + i;
    const float v = (q >= 0 && q < n_in) ? xb[q] : 0.f;
    acc = fmaf(kp[i], v, acc);
  }
  y[(long)blockIdx.y * y_stride + n] = acc;
}

// ---- backward: the exact transpose, in gather form ----------------------------------------------------------------
// dx[q] = sum over (j, p), ascending n = j neu + p < n_out, of k[p][q + width - j orig] * dy[n], for the phase
// periods j whose tap index i = q + width - j orig lies in [0, taps): j = jhi - m with jhi = (q + width) / orig and
// m < M = ceil(taps / orig), so i = (q + width) % orig + m orig.  One thread owns one q and runs one fmaf chain, m
// descending (j ascending) and p ascending: the result is a function of the row alone.  A workgroup takes RS_TILE
// consecutive q.  It stages the dy span its periods cover in LDS: for a large orig the lanes of a wave share j and
// the read is a broadcast, for a small orig (8 kHz -> 24 kHz: orig 1) every lane has its own j and reads dy at
// stride neu, which LDS serves and a global load would not coalesce.  The taps come from the forward's own table:
// for fixed (m, p) neighbouring q read neighbouring k[p][i], a coalesced load that L1/L2 serve.
constexpr int RS_TILE = 256;
constexpr int RS_MAX_SPAN = 16384;                      // 64 KB of LDS per workgroup

// floats of dy one backward tile stages: the periods of RS_TILE consecutive q, plus the M - 1 before the first
long backward_span(int orig, int neu, int taps) {
  const long m = (taps + orig - 1) / orig;
  return ((long)(RS_TILE + orig - 2) / orig + m) * neu;
}

__device__ __forceinline__ void resample_backward_tile(const float* __restrict__ dyb, int n_out,
                                                       float* __restrict__ dxb, int n_in, int q0,
                                                       const float* __restrict__ k, int orig, int neu, int width,
                                                       int taps, float* ds) {
  const int q_last = min(q0 + RS_TILE, n_in) - 1;
  const int M = (taps + orig - 1) / orig;
  const int j0 = max(0, (q0 + width) / orig - (M - 1));
  const int n_lo = j0 * neu;
  const int span = (int)min((long)((q_last + width) / orig + 1) * neu, (long)n_out) - n_lo;
  for (int s = threadIdx.x; s < span; s += RS_TILE) ds[s] = dyb[n_lo + s];
  __syncthreads();
  const int q = q0 + threadIdx.x;
  if (q >= n_in) return;
  const int jhi = (q + width) / orig, r = q + width - jhi * orig;
  float acc = 0.f;
  for (int m = M - 1; m >= 0; --m) {
    const int j = jhi - m, i = r + m * orig;
    if (j < 0 || i >= taps) continue;
    const long n0 = (long)j * neu;
    const int pe = (int)min((long)neu, (long)n_out - n0);  // the n < n_out cut; <= 0 past the last period
    const float* kp = k + i;
    const float* dp = ds + (n0 - n_lo);
    for (int p = 0; p < pe; ++p) acc = fmaf(kp[(long)p * taps], dp[p], acc);
  }
  dxb[q] = acc;
}

__global__ __launch_bounds__(RS_TILE) void resample_backward_kernel(const float* __restrict__ dy, long dy_stride,
                                                                    int n_out, float* __restrict__ dx, long dx_stride,
                                                                    int n_in, const float* __restrict__ k, int orig,
                                                                    int neu, int width, int taps) {
  extern __shared__ float ds[];
  resample_backward_tile(dy + (long)blockIdx.y * dy_stride, n_out, dx + (long)blockIdx.y * dx_stride, n_in,
                         blockIdx.x * RS_TILE, k, orig, neu, width, taps, ds);
}

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// The [neu][taps] tap table of torchaudio's _get_sinc_resample_kernel for the reduced ratio orig -> neu, and its
// width / taps.  Shared by the single-rate and the multi-rate plans, so both hold the same fp32 taps.
void sinc_taps(int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, int* orig_out, int* neu_out,
               int* width_out, int* taps_out, std::vector<float>& k) {
  const int g = gcd_i(orig_freq, new_freq);
  const int orig = orig_freq / g, neu = new_freq / g;
  const double base_freq = (double)(orig < neu ? orig : neu) * (double)rolloff;
  const int width = (int)ceil((double)lowpass_filter_width * orig / base_freq);
  const int taps = 2 * width + orig;
  k.assign((size_t)neu * taps, 0.f);
  const double scale = base_freq / orig;
  for (int p = 0; p < neu; ++p)
    for (int i = 0; i < taps; ++i) {
      double t = ((double)(-p) / neu + (double)(i - width) / orig) * base_freq;
      if (t < -lowpass_filter_width) t = -lowpass_filter_width;
      if (t > lowpass_filter_width) t = lowpass_filter_width;
      const double c = cos(t * M_PI / lowpass_filter_width / 2.0);
      const double window = c * c;
      const double tp = t * M_PI;
      const double sinc = (tp == 0.0) ? 1.0 : sin(tp) / tp;
      k[(size_t)p * taps + i] = (float)(sinc * window * scale);
    }
  *orig_out = orig; *neu_out = neu; *width_out = width; *taps_out = taps;
}

}  // namespace

extern "C" int pe_resample_plan_create(pe_resample_plan** plan_out, int orig_freq, int new_freq,
                                       int lowpass_filter_width, float rolloff) {
  if (!plan_out || orig_freq <= 0 || new_freq <= 0 || lowpass_filter_width <= 0 || !(rolloff > 0.f)) return PE_E_ARG;
  int orig, neu, width, taps;
  std::vector<float> k;
  sinc_taps(orig_freq, new_freq, lowpass_filter_width, rolloff, &orig, &neu, &width, &taps, k);
  float* d = nullptr;
  PE_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&d), k.size() * sizeof(float)));
  hipError_t e = hipMemcpy(d, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); return (int)e; }
  pe_resample_plan* pl = new pe_resample_plan{orig, neu, width, taps, d};
  *plan_out = pl;
  return PE_OK;
}

extern "C" int pe_resample_plan_destroy(pe_resample_plan* plan) {
  if (!plan) return PE_E_ARG;
  hipError_t e = hipFree(plan->d_kernel);
  delete plan;
  return (int)e;
}

/* ceil(new * n_in / orig) with the reduced ratio */
extern "C" long pe_resample_out_len(const pe_resample_plan* plan, long n_in) {
  if (!plan || n_in < 0) return PE_E_ARG;
  return (n_in * plan->neu + plan->orig - 1) / plan->orig;
}

extern "C" int pe_resample_forward(const pe_resample_plan* plan, const float* x, int batch, int n_in, long x_stride,
                                   float* y, long y_stride, int n_out, void* stream) {
  if (!plan || !x || !y || batch < 0 || n_in < 0 || n_out < 0 || x_stride < n_in || y_stride < n_out) return PE_E_ARG;
  if (batch == 0 || n_out == 0) return PE_OK;
  if (batch > 65535) return PE_E_UNSUPPORTED;
  if ((long)n_out > pe_resample_out_len(plan, n_in)) return PE_E_ARG;
  hipLaunchKernelGGL(resample_kernel, dim3(pe_cdiv(n_out, 256), batch), dim3(256), 0, pe_stream(stream), x, x_stride,
                     n_in, y, y_stride, n_out, plan->d_kernel, plan->orig, plan->neu, plan->width, plan->taps);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_resample_backward(const pe_resample_plan* plan, const float* dy, int batch, int n_out, long dy_stride,
                                    float* dx, long dx_stride, int n_in, void* stream) {
  if (!plan || !dy || !dx || batch < 0 || n_in < 0 || n_out < 0 || dy_stride < n_out || dx_stride < n_in) return PE_E_ARG;
  if ((long)n_out > pe_resample_out_len(plan, n_in)) return PE_E_ARG;
  if (batch == 0 || n_in == 0) return PE_OK;
  const long span = backward_span(plan->orig, plan->neu, plan->taps);
  if (batch > 65535 || span > RS_MAX_SPAN) return PE_E_UNSUPPORTED;
  hipLaunchKernelGGL(resample_backward_kernel, dim3(pe_cdiv(n_in, RS_TILE), batch), dim3(RS_TILE),
                     (size_t)span * sizeof(float), pe_stream(stream), dy, dy_stride, n_out, dx, dx_stride, n_in,
                     plan->d_kernel, plan->orig, plan->neu, plan->width, plan->taps);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

// ---- multi-rate ragged resampler --------------------------------------------------------------------------------
// One launch resamples a batch whose rows come at different source rates.  Row r (input at x + x_off[r], n_in[r]
// samples, source rate rates[rate_idx[r]]) writes its out_len outputs at y + r * y_stride and zeros from there to
// y_width.  The grid is the flat list of (output tile, row) items over [0, y_width): a tile past a row's output
// only stores zeros, so the padding of short rows costs a store and no taps.  A computing tile stages the input
// span its 256 outputs read in LDS (zero outside the row), then runs resample_kernel's fmaf chain over the same
// fp32 taps in the same order, so each row equals pe_resample_forward on that row alone bit for bit.  A rate
// equal to the target copies (torchaudio returns the input unchanged).

struct pe_resample_rate {
  int orig, neu, width, taps;     // reduced ratio; neu == 0: copy
  long koff;                      // offset of the [neu][taps] table in floats
};

namespace {

constexpr int RS_MAX_RATES = 16;

struct rs_rates { pe_resample_rate r[RS_MAX_RATES]; };  // kernel argument (byref kernarg: no scratch)

}  // namespace

struct pe_resample_ragged_plan {
  int n_rates, span;              // span: largest LDS input span of one tile, floats
  rs_rates rates;
  float* d_table;                 // every non-copy rate's [neu][taps] table; null when all rates copy
  long bspan;                     // largest LDS dy span of one backward tile, floats (may pass RS_MAX_SPAN)
};

namespace {

__global__ __launch_bounds__(RS_TILE) void resample_ragged_kernel(const float* __restrict__ x,
                                                                  const long* __restrict__ x_off,
                                                                  const int* __restrict__ n_in,
                                                                  const int* __restrict__ rate_idx,
                                                                  float* __restrict__ y, long y_stride, int y_width,
                                                                  const float* __restrict__ table, rs_rates rates) {
  extern __shared__ float xs[];
  const int row = blockIdx.y;
  const int n0 = blockIdx.x * RS_TILE, n = n0 + threadIdx.x;
  const pe_resample_rate d = rates.r[rate_idx[row]];
  const int nin = n_in[row];
  const int n_out = d.neu ? (int)(((long)nin * d.neu + d.orig - 1) / d.orig) : nin;
  float* yb = y + (long)row * y_stride;
  const float* xb = x + x_off[row];
  if (n0 >= n_out || d.neu == 0) {                      // padding tile, or a copied row
    if (n < y_width) yb[n] = n < n_out ? xb[n] : 0.f;
    return;
  }
  const int n_last = min(n0 + RS_TILE, n_out) - 1;
  const int lo = (n0 / d.neu) * d.orig - d.width;
  const int span = (n_last / d.neu) * d.orig - d.width + d.taps - lo;
  for (int s = threadIdx.x; s < span; s += RS_TILE) {
    const int q = lo + s;
    xs[s] = (q >= 0 && q < nin) ? xb[q] : 0.f;
  }
  __syncthreads();
  if (n >= y_width) return;
  if (n >= n_out) { yb[n] = 0.f; return; }
  const int j = n / d.neu, p = n - j * d.neu;
  const float* kp = table + d.koff + (long)p * d.taps;
  const float* xr = xs + (j * d.orig - d.width - lo);
  float acc = 0.f;
  for (int i = 0; i < d.taps; ++i) acc = fmaf(kp[i], xr[i], acc);
  yb[n] = acc;
}

// Backward of the launch above.  Row r reads its own out_len values at dy + r * dy_stride and writes n_in[r]
// gradients at dx + x_off[r], where the forward read its input; with dx_width > 0 (padded rows) it also writes zeros
// from n_in[r] to dx_width, with dx_width == 0 (packed rows) nothing else.  A computing tile is
// resample_backward_tile, as in resample_backward_kernel: the same bits as pe_resample_backward on the row alone.
__global__ __launch_bounds__(RS_TILE) void resample_ragged_backward_kernel(const float* __restrict__ dy, long dy_stride,
                                                                           const long* __restrict__ x_off,
                                                                           const int* __restrict__ n_in,
                                                                           const int* __restrict__ rate_idx,
                                                                           float* __restrict__ dx, int dx_width,
                                                                           const float* __restrict__ table,
                                                                           rs_rates rates) {
  extern __shared__ float ds[];
  const int row = blockIdx.y;
  const int q0 = blockIdx.x * RS_TILE, q = q0 + threadIdx.x;
  const pe_resample_rate d = rates.r[rate_idx[row]];
  const int nin = n_in[row];
  const float* dyb = dy + (long)row * dy_stride;
  float* dxb = dx + x_off[row];
  if (q0 >= nin || d.neu == 0) {                        // padding tile, or a copied row
    if (q < nin) dxb[q] = dyb[q];
    else if (q < dx_width) dxb[q] = 0.f;
    return;
  }
  const int n_out = (int)(((long)nin * d.neu + d.orig - 1) / d.orig);
  resample_backward_tile(dyb, n_out, dxb, nin, q0, table + d.koff, d.orig, d.neu, d.width, d.taps, ds);
  if (q >= nin && q < dx_width) dxb[q] = 0.f;
}

long ragged_out_len(const pe_resample_rate& d, long n_in) {
  return d.neu ? (n_in * d.neu + d.orig - 1) / d.orig : n_in;
}

}  // namespace

extern "C" int pe_resample_ragged_plan_create(pe_resample_ragged_plan** plan_out, const int* orig_freqs, int n_rates,
                                              int new_freq, int lowpass_filter_width, float rolloff) {
  if (!plan_out || !orig_freqs || n_rates <= 0 || n_rates > RS_MAX_RATES || new_freq <= 0 || lowpass_filter_width <= 0 || !(rolloff > 0.f))
    return PE_E_ARG;
  for (int r = 0; r < n_rates; ++r)
    if (orig_freqs[r] <= 0) return PE_E_ARG;
  rs_rates rates = {};
  std::vector<float> all, k;
  int span = 0;
  long bspan = 0;
  for (int r = 0; r < n_rates; ++r) {
    pe_resample_rate& d = rates.r[r];
    if (orig_freqs[r] == new_freq) { d = pe_resample_rate{1, 0, 0, 0, 0}; continue; }
    sinc_taps(orig_freqs[r], new_freq, lowpass_filter_width, rolloff, &d.orig, &d.neu, &d.width, &d.taps, k);
    d.koff = (long)all.size();
    all.insert(all.end(), k.begin(), k.end());
    // input span of a tile: (n_last / neu - n0 / neu) <= (neu - 1 + RS_TILE - 1) / neu phase periods, plus the taps
    const long s = (long)((d.neu + RS_TILE - 2) / d.neu) * d.orig + d.taps;
    if (s > RS_MAX_SPAN) return PE_E_UNSUPPORTED;
    if (s > span) span = (int)s;
    const long b = backward_span(d.orig, d.neu, d.taps);
    if (b > bspan) bspan = b;
  }
  float* d = nullptr;                                   // a plan of copies only touches no device
  if (!all.empty()) {
    PE_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&d), all.size() * sizeof(float)));
    hipError_t e = hipMemcpy(d, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return (int)e; }
  }
  *plan_out = new pe_resample_ragged_plan{n_rates, span, rates, d, bspan};
  return PE_OK;
}

extern "C" int pe_resample_ragged_plan_destroy(pe_resample_ragged_plan* plan) {
  if (!plan) return PE_E_ARG;
  hipError_t e = plan->d_table ? hipFree(plan->d_table) : hipSuccess;
  delete plan;
  return (int)e;
}

/* output length of an n_in-sample row at rate index rate_index */
extern "C" long pe_resample_ragged_out_len(const pe_resample_ragged_plan* plan, int rate_index, long n_in) {
  if (!plan || rate_index < 0 || rate_index >= plan->n_rates || n_in < 0) return PE_E_ARG;
  return ragged_out_len(plan->rates.r[rate_index], n_in);
}

extern "C" int pe_resample_ragged_forward(const pe_resample_ragged_plan* plan, const float* x, const long* x_off,
                                          const int* n_in, const int* rate_idx, const int* host_n_in,
                                          const int* host_rate_idx, int batch, float* y, long y_stride, int y_width,
                                          void* stream) {
  if (!plan || !x || !x_off || !n_in || !rate_idx || !host_n_in || !host_rate_idx || !y || batch < 0 ||
      y_width < 0 || y_stride < y_width)
    return PE_E_ARG;
  for (int r = 0; r < batch; ++r) {
    if (host_rate_idx[r] < 0 || host_rate_idx[r] >= plan->n_rates || host_n_in[r] < 0) return PE_E_ARG;
    if (ragged_out_len(plan->rates.r[host_rate_idx[r]], host_n_in[r]) > y_width) return PE_E_ARG;
  }
  if (batch == 0 || y_width == 0) return PE_OK;
  if (batch > 65535) return PE_E_UNSUPPORTED;
  hipLaunchKernelGGL(resample_ragged_kernel, dim3(pe_cdiv(y_width, RS_TILE), batch), dim3(RS_TILE),
                     (size_t)plan->span * sizeof(float), pe_stream(stream), x, x_off, n_in, rate_idx, y, y_stride,
                     y_width, plan->d_table, plan->rates);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_resample_ragged_backward(const pe_resample_ragged_plan* plan, const float* dy, long dy_stride,
                                           const long* x_off, const int* n_in, const int* rate_idx,
                                           const int* host_n_in, const int* host_rate_idx, int batch, float* dx,
                                           int dx_width, void* stream) {
  if (!plan || !dy || !x_off || !n_in || !rate_idx || !host_n_in || !host_rate_idx || !dx || batch < 0 ||
      dx_width < 0 || dy_stride < 0)
    return PE_E_ARG;
  int cover = dx_width;                                 // samples of a row the grid spans
  for (int r = 0; r < batch; ++r) {
    if (host_rate_idx[r] < 0 || host_rate_idx[r] >= plan->n_rates || host_n_in[r] < 0) return PE_E_ARG;
    if (ragged_out_len(plan->rates.r[host_rate_idx[r]], host_n_in[r]) > dy_stride) return PE_E_ARG;
    if (dx_width > 0 && host_n_in[r] > dx_width) return PE_E_ARG;
    if (host_n_in[r] > cover) cover = host_n_in[r];
  }
  if (batch == 0 || cover == 0) return PE_OK;
  if (batch > 65535 || plan->bspan > RS_MAX_SPAN) return PE_E_UNSUPPORTED;
  hipLaunchKernelGGL(resample_ragged_backward_kernel, dim3(pe_cdiv(cover, RS_TILE), batch), dim3(RS_TILE),
                     (size_t)plan->bspan * sizeof(float), pe_stream(stream), dy, dy_stride, x_off, n_in, rate_idx, dx,
                     dx_width, plan->d_table, plan->rates);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
