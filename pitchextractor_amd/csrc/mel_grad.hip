// Backward of the fused mel front end (mel.hip) with respect to the waveform, for gfx950.
//
// Given G = dL/dout at the forward's strides, the spectrum X_t and the mel M_t of every frame are RECOMPUTED from the
// wave (nothing is stored by the forward), then dM = G or G / (std (eps + M)), dP = F dM (the filterbank by bin: at
// most two filters each), Y = dP X with the two real bins doubled, u_t = the unnormalised inverse real transform of Y
// (real_fft_pack + an inverse 512-point transform, times 2), and d xp[t hop + j] += w[j] u_t[j]; the reflect padding
// is transposed at the end.  Two launches, no atomics, every element of grad_wave written exactly once:
//   frames: one workgroup per (row, block of FB consecutive SOURCE frames counted from the row's frame 0).  Each of
//           the 4 waves takes one frame of a round of 4 through a wave-private LDS region; after every round the
//           workgroup adds the round's windowed frames into an LDS segment of (FB - 1) hop + 1024 floats, one thread
//           per position, frames in ascending order; the segment goes to the block's workspace slab.
//   gather: one thread per output sample sums, in ascending block order, the slab entries that cover padded position
//           n + 512 and then its at most two reflect images.
// Block boundaries and every order of summation are functions of the row alone (its length, its crop), so a row's
// gradient is the same bits alone, in any batch and at any stride.
#include <math.h>
#include "common.h"
#include "dsp.h"
#include "mel_plan.h"

using namespace pe;

namespace {

constexpr int kNfft = 1024;
constexpr int kHalf = 512;                 // complex FFT length
constexpr int kMaxParts = 6;               // 8-tap chunks per mel filter (mel.hip)
constexpr int kWaveBuf = kNfft + 256;      // floats of a wave's region: Z | P, chunk sums | Y | w u, then dM[256]
constexpr int kPartAt = 520;               // chunk sums behind the 513 (+7 zero) powers
constexpr long kMaxSamples = 1L << 30;     // padded positions and their mirror images stay far inside an int
constexpr size_t kMaxLds = 160 * 1024;

struct MelGradArgs {
  const float* wave;
  long wave_stride;
  int n_samples;               // row length (fixed batch) / longest row (ragged): the rows of grad_wave
  const int* n_samples_arr;    // optional [batch]
  const int* frame_start;      // optional [batch]
  const float* grad_out;
  long g_sb, g_sm, g_st;
  int out_frames;
  int hop, n_mels, n_pairs, log_mode;
  float log_eps, inv_std;
  const float* win;
  const float2* tw512;
  const float2* tw1024;
  const int* fb_idx;
  const float* fb_w;
  const int2* tfb_m;
  const float2* tfb_w;
  int fb;                      // source frames per block (a multiple of 4)
  int seg_len;                 // (fb - 1) * hop + 1024
  long seg_stride;             // floats per slab
  int nb_ws;                   // slabs per row
  float* ws;
  float* grad_wave;
  long grad_wave_stride;
};

// What of a row carries gradient: its samples and the source frames [lo, hi) that the output shows.
struct RowSpan { int n, lo, hi; };

__device__ __forceinline__ RowSpan row_span(const MelGradArgs& a, int b) {
  RowSpan s;
  s.n = a.n_samples_arr ? min(a.n_samples_arr[b], a.n_samples) : a.n_samples;
  // reflect padding needs more than n_fft/2 samples; the forward shows shorter rows as padding only
  const int n_valid = s.n > kHalf ? 1 + s.n / a.hop : 0;
  s.lo = a.frame_start ? max(a.frame_start[b], 0) : 0;
  s.hi = (int)min((long)n_valid, (long)s.lo + a.out_frames);
  return s;
}

__global__ __launch_bounds__(256, 3) void mel_bwd_frames_kernel(const MelGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_seg = reinterpret_cast<float*>(smem);                      // [seg_stride]
  float* s_wave = s_seg + a.seg_stride;                               // [4][kWaveBuf]
  float2* s_tw = reinterpret_cast<float2*>(s_wave + 4 * kWaveBuf);    // [512]
  float* s_fbw = reinterpret_cast<float*>(s_tw + kHalf);              // [n_pairs][8]
  int* s_fbi = reinterpret_cast<int*>(s_fbw + a.n_pairs * 8);         // k0[n_pairs] | first[n_mels] | cnt[n_mels]

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y, hop = a.hop, n_mels = a.n_mels;
  const RowSpan row = row_span(a, b);
  const int f_blk = (row.lo / a.fb + (int)blockIdx.x) * a.fb;         // first source frame of this block
  if (row.lo >= row.hi || f_blk >= row.hi) return;                    // no frame here: gather never reads this slab

  for (int j = tid; j < a.seg_len; j += 256) s_seg[j] = 0.0f;
  for (int j = tid; j < kHalf; j += 256) s_tw[j] = a.tw512[j];
  for (int j = tid; j < a.n_pairs * 8; j += 256) s_fbw[j] = a.fb_w[j];
  for (int j = tid; j < a.n_pairs + 2 * n_mels; j += 256) s_fbi[j] = a.fb_idx[j];
  float2 win[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = 64 * r + lane;
    win[r] = make_float2(a.win[2 * n], a.win[2 * n + 1]);
  }
  float* buf = s_wave + wv * kWaveBuf;
  float2* Z = reinterpret_cast<float2*>(buf);
  float* P = buf;
  float* part = buf + kPartAt;
  float* dM = buf + kNfft;
  const float* wsrc = a.wave + (long)b * a.wave_stride;
  const unsigned long wsrc_addr = reinterpret_cast<unsigned long>(wsrc);
  const long N = row.n;
  const float* gsrc = a.grad_out + (long)b * a.g_sb;
  __syncthreads();

  for (int it = 0; it < a.fb / 4; ++it) {
    const int f_round = f_blk + 4 * it;
    if (f_round + 4 <= row.lo || f_round >= row.hi) continue;        // workgroup-uniform: no frame in this round
    const int f = f_round + wv;
    if (f >= row.lo && f < row.hi) {                                  // wave-uniform
      // ---- the frame, windowed, as 512 complex points (the forward's loads)
      const long base = (long)f * hop - kHalf;
      if (base >= 0 && base + kNfft <= N && ((wsrc_addr + 4 * (unsigned long)base) & 7) == 0) {
        const float2* fr = reinterpret_cast<const float2*>(wsrc + base);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const float2 x = fr[64 * r + lane];
          Z[64 * r + lane] = make_float2(x.x * win[r].x, x.y * win[r].y);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          float x2[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            long g = base + 2 * (64 * r + lane) + e;
            if (g < 0) g = -g;
            if (g >= N) g = 2 * (N - 1) - g;
            x2[e] = (g >= 0 && g < N) ? wsrc[g] : 0.0f;
          }
          Z[64 * r + lane] = make_float2(x2[0] * win[r].x, x2[1] * win[r].y);
        }
      }
      wave_lds_sync();
      fft_lds<9, false, 64>(Z, s_tw, lane);

      // ---- X[k] and X[512 - k] for k = lane + 64 j, and X[256], held in registers
      float2 xk[4], xn[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        float2 e, o;
        const float2 t = real_fft_bin(Z, a.tw1024[k], kHalf, k, e, o);
        xk[j] = cadd(e, t);
        xn[j] = conj2(csub(e, t));
      }
      float2 x256;
      {
        float2 e, o;
        const float2 t = real_fft_bin(Z, a.tw1024[256], kHalf, 256, e, o);
        x256 = cadd(e, t);
      }
      wave_lds_sync();                                                // Z is read: P and the chunk sums overwrite it

      // ---- dM
      const long g_at = (long)(f - row.lo) * a.g_st;
      if (a.log_mode) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = lane + 64 * j;
          P[k] = xk[j].x * xk[j].x + xk[j].y * xk[j].y;
          P[kNfft / 2 - k] = xn[j].x * xn[j].x + xn[j].y * xn[j].y;
        }
        if (lane == 0) P[256] = x256.x * x256.x + x256.y * x256.y;
        else if (lane < 8) P[kNfft / 2 + lane] = 0.0f;                // zero tail read by the padded 8-tap chunks
        wave_lds_sync();
        for (int id = lane; id < a.n_pairs; id += 64) {
          const int k0 = s_fbi[id];
          const float4 w0 = *reinterpret_cast<const float4*>(s_fbw + id * 8);
          const float4 w1 = *reinterpret_cast<const float4*>(s_fbw + id * 8 + 4);
          float acc = w0.x * P[k0];
          acc = fmaf(w0.y, P[k0 + 1], acc); acc = fmaf(w0.z, P[k0 + 2], acc); acc = fmaf(w0.w, P[k0 + 3], acc);
          acc = fmaf(w1.x, P[k0 + 4], acc); acc = fmaf(w1.y, P[k0 + 5], acc); acc = fmaf(w1.z, P[k0 + 6], acc);
          acc = fmaf(w1.w, P[k0 + 7], acc);
          part[id] = acc;
        }
        wave_lds_sync();
        for (int m = lane; m < n_mels; m += 64) {
          const int first = s_fbi[a.n_pairs + m], cnt = s_fbi[a.n_pairs + n_mels + m];
          float acc = 0.0f;
#pragma unroll
          for (int j = 0; j < kMaxParts; ++j) acc += (j < cnt) ? part[first + j] : 0.0f;
          dM[m] = gsrc[(long)m * a.g_sm + g_at] * (a.inv_std / (a.log_eps + acc));
        }
      } else {
        for (int m = lane; m < n_mels; m += 64) dM[m] = gsrc[(long)m * a.g_sm + g_at];
      }
      wave_lds_sync();

      // ---- Y = dP X (the real bins 0 and 512 doubled), packed for the inverse 512-point transform
      auto d_power = [&](int k) {
        const int2 m2 = a.tfb_m[k];
        const float2 w2 = a.tfb_w[k];
        return fmaf(w2.y, dM[m2.y], w2.x * dM[m2.x]);
      };
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        const float dk = d_power(k), dn = d_power(kHalf - k);
        float2 yk = make_float2(dk * xk[j].x, dk * xk[j].y), yn = make_float2(dn * xn[j].x, dn * xn[j].y);
        if (k == 0) {
          yk = make_float2(2.0f * yk.x, 0.0f);
          yn = make_float2(2.0f * yn.x, 0.0f);
        }
        const float2 w = a.tw1024[k];
        Z[k] = real_fft_pack(yk, conj2(yn), w);
        // exp(-2 pi i (512 - k) / 1024) = -conj(w)
        if (k != 0) Z[kHalf - k] = real_fft_pack(yn, conj2(yk), make_float2(-w.x, w.y));
      }
      if (lane == 0) {
        const float d = d_power(256);
        const float2 y = make_float2(d * x256.x, d * x256.y);
        Z[256] = real_fft_pack(y, conj2(y), a.tw1024[256]);
      }
      wave_lds_sync();
      fft_lds<9, true, 64>(Z, s_tw, lane);

      // ---- u = 2 z (even samples in the real parts, odd ones in the imaginary parts), windowed, in place
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float2 z = Z[64 * r + lane];
        Z[64 * r + lane] = make_float2(2.0f * z.x * win[r].x, 2.0f * z.y * win[r].y);
      }
    }
    __syncthreads();
    // ---- overlap-add of the round: one thread per position of the segment, frames in ascending order
    const int seg0 = 4 * it * hop;
    for (int s = tid; s < 3 * hop + kNfft; s += 256) {
      float acc = s_seg[seg0 + s];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int off = s - w * hop, fw = f_round + w;
        if (fw >= row.lo && fw < row.hi && off >= 0 && off < kNfft) acc += s_wave[w * kWaveBuf + off];
      }
      s_seg[seg0 + s] = acc;
    }
    __syncthreads();
  }

  float* dst = a.ws + ((long)b * a.nb_ws + blockIdx.x) * a.seg_stride;
  for (int s = tid; s < a.seg_len; s += 256) dst[s] = s_seg[s];
}

__global__ __launch_bounds__(256) void mel_bwd_gather_kernel(const MelGradArgs a) {
  const int b = blockIdx.y;
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_samples) return;
  const RowSpan row = row_span(a, b);
  float* dst = a.grad_wave + (long)b * a.grad_wave_stride;
  if (n >= row.n || row.lo >= row.hi) {                 // past the row's end, or a row without a frame
    dst[n] = 0.0f;
    return;
  }
  const long block_hop = (long)a.fb * a.hop;            // >= 1024: at most two blocks cover a padded position
  const long j0 = row.lo / a.fb;
  const float* slabs = a.ws + (long)b * a.nb_ws * a.seg_stride;
  auto at = [&](long p) {                               // d xp[p]: the covering blocks, ascending
    const long jh = p / block_hop;
    float acc = 0.0f;
    for (long j = jh - 1; j <= jh; ++j) {
      const long off = p - j * block_hop;
      if (j < j0 || j * a.fb >= row.hi || j - j0 >= a.nb_ws || off >= a.seg_len) continue;
      acc += slabs[(j - j0) * a.seg_stride + off];
    }
    return acc;
  };
  const long N = row.n;
  float g = at(n + kHalf);
  if (n >= 1 && n <= kHalf) g += at(kHalf - n);
  if (n >= N - kHalf - 1 && n <= N - 2) g += at(kHalf + 2 * (N - 1) - n);
  dst[n] = g;
}

// frames per block: about 4800 samples of hop per block (16 frames at hop 300), a multiple of 4, so that the
// (FB - 1) hop + 1024 floats of the segment stay near 23 KB and FB hop >= 1024
int grad_fb(int hop) {
  const int fb = pe_cdiv(4800, hop) < 4 ? 4 : pe_cdiv(4800, hop);
  return (fb + 3) & ~3;
}
long grad_seg_len(int hop) { return (long)(grad_fb(hop) - 1) * hop + kNfft; }
long grad_seg_stride(int hop) { return (grad_seg_len(hop) + 3) & ~3L; }
// slabs per row: the blocks that hold one of out_frames consecutive frames of a row of max_samples
long grad_slabs(int hop, int max_samples, int out_frames) {
  const int fb = grad_fb(hop);
  const long of_row = pe_cdiv(1 + (long)max_samples / hop, fb), of_crop = pe_cdiv(out_frames, fb) + 1L;
  return of_row < of_crop ? of_row : of_crop;
}

int mel_bwd_launch(const pe_mel_plan* plan, const float* wave, int batch, int n_samples, long wave_stride,
                   const int* n_samples_arr, const int* frame_start, bool ragged, const float* grad_out, long g_sb,
                   long g_sm, long g_st, int out_frames, int log_mode, float log_eps, float mean, float std,
                   float* grad_wave, long grad_wave_stride, void* workspace, size_t workspace_bytes, void* stream) {
  (void)mean;
  if (!plan || !wave || !grad_out || !grad_wave || !workspace || (ragged && !n_samples_arr)) return PE_E_ARG;
  if (batch <= 0 || n_samples <= 0 || out_frames <= 0 || std == 0.0f || plan->hop <= 0) return PE_E_ARG;
  if ((!ragged && n_samples <= kHalf) || wave_stride < n_samples || grad_wave_stride < n_samples) return PE_E_ARG;
  if (batch > 65535 || n_samples > kMaxSamples) return PE_E_UNSUPPORTED;
  const int hop = plan->hop;
  const long seg_stride = grad_seg_stride(hop);
  const size_t lds = ((size_t)(seg_stride + 4 * kWaveBuf) * 4 + kHalf * 8 + (size_t)plan->n_pairs * 8 * 4 +
                      (size_t)(plan->n_pairs + 2 * plan->n_mels) * 4 + 15) & ~(size_t)15;
  if (lds > kMaxLds || plan->n_mels > 256 || plan->n_pairs > kNfft - kPartAt) return PE_E_UNSUPPORTED;
  if (workspace_bytes < pe_mel_backward_workspace_bytes(plan, batch, n_samples, out_frames)) return PE_E_WORKSPACE;
  if (!plan->d_tfb_m) return PE_E_UNSUPPORTED;           // a bin with more than two filters

  MelGradArgs a;
  a.wave = wave; a.wave_stride = wave_stride; a.n_samples = n_samples;
  a.n_samples_arr = n_samples_arr; a.frame_start = frame_start;
  a.grad_out = grad_out; a.g_sb = g_sb; a.g_sm = g_sm; a.g_st = g_st; a.out_frames = out_frames;
  a.hop = hop; a.n_mels = plan->n_mels; a.n_pairs = plan->n_pairs; a.log_mode = log_mode;
  a.log_eps = log_eps; a.inv_std = 1.0f / std;
  a.win = plan->d_win; a.tw512 = plan->d_tw512; a.tw1024 = plan->d_tw1024;
  a.fb_idx = plan->d_fb_idx; a.fb_w = plan->d_fb_w; a.tfb_m = plan->d_tfb_m; a.tfb_w = plan->d_tfb_w;
  a.fb = grad_fb(hop); a.seg_len = (int)grad_seg_len(hop); a.seg_stride = seg_stride;
  a.nb_ws = (int)grad_slabs(hop, n_samples, out_frames);
  a.ws = reinterpret_cast<float*>(workspace);
  a.grad_wave = grad_wave; a.grad_wave_stride = grad_wave_stride;

  if (lds > 64 * 1024)                                   // a long hop: past the default limit, on this device
    PE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mel_bwd_frames_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
  hipLaunchKernelGGL(mel_bwd_frames_kernel, dim3(a.nb_ws, batch), dim3(256), lds, pe_stream(stream), a);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(mel_bwd_gather_kernel, dim3(pe_cdiv(n_samples, 256), batch), dim3(256), 0, pe_stream(stream), a);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

}  // namespace

extern "C" size_t pe_mel_backward_workspace_bytes(const pe_mel_plan* plan, int batch, int max_samples,
                                                  int out_frames) {
  if (!plan || plan->hop <= 0 || batch <= 0 || max_samples <= 0 || out_frames <= 0) return 0;
  return (size_t)batch * (size_t)grad_slabs(plan->hop, max_samples, out_frames) *
         (size_t)grad_seg_stride(plan->hop) * sizeof(float);
}

extern "C" int pe_mel_backward(const pe_mel_plan* plan, const float* wave, int batch, int n_samples, long wave_stride,
                               const float* grad_out, long g_sb, long g_sm, long g_st, int out_frames, int log_mode,
                               float log_eps, float mean, float std, float* grad_wave, long grad_wave_stride,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return mel_bwd_launch(plan, wave, batch, n_samples, wave_stride, nullptr, nullptr, false, grad_out, g_sb, g_sm, g_st,
                        out_frames, log_mode, log_eps, mean, std, grad_wave, grad_wave_stride, workspace,
                        workspace_bytes, stream);
}

extern "C" int pe_mel_backward_ragged(const pe_mel_plan* plan, const float* wave, int batch, int max_samples,
                                      long wave_stride, const int* n_samples, const int* frame_start,
                                      const float* grad_out, long g_sb, long g_sm, long g_st, int out_frames,
                                      int log_mode, float log_eps, float mean, float std, float* grad_wave,
                                      long grad_wave_stride, void* workspace, size_t workspace_bytes, void* stream) {
  return mel_bwd_launch(plan, wave, batch, max_samples, wave_stride, n_samples, frame_start, true, grad_out, g_sb,
                        g_sm, g_st, out_frames, log_mode, log_eps, mean, std, grad_wave, grad_wave_stride, workspace,
                        workspace_bytes, stream);
}
