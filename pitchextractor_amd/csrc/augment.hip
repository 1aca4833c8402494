// Training-time augmentation on ragged batches: a cascade of up to 8 biquads per row, each row with its own
// coefficients, evaluated as a parallel scan in double.  Pinned by the float64 restatement in tests/augment_ref.py.
//
// Definition: the row's float32 samples widened to double run through the row's stages in transposed direct form II,
//   y = b0 x + z1;  z1 = b1 x - a1 y + z2;  z2 = b2 x - a2 y,
// from a zero state, without a clamp or a rounding between two stages, and are rounded once to float32 at the end:
// scipy.signal.sosfilt in float64 followed by a cast.  (pe_stress_biquad of stress.hip is torchaudio's lfilter: a clamp
// and a float32 store behind every stage, which is why that one walks its rows sample by sample.)
//
// One workgroup of kThreads per row walks the row in blocks of kBlock samples counted from the row's own first sample;
// lane t owns the kPiece consecutive samples [t kPiece, (t + 1) kPiece) of a block, in registers.  Per stage:
//   1. every lane runs its piece from a zero state and keeps the end state e_t (two doubles);
//   2. with A = {{-a1, 1}, {-a2, 0}} the state's homogeneous step and M = A^kPiece, the true end states obey
//      s_t = M s_(t-1) + e_t.  Inside a wave that is a log-step scan over the lanes with M^(2^j), by shuffles; the four
//      wave ends meet in LDS and are chained in order behind the block's carry, c_(w+1) = M^64 c_w + E_w; lane l of
//      wave w then starts from (its neighbour's scanned end) + M^l c_w, M^l by the bits of l;
//   3. every lane runs its piece again from that state, which replaces the piece by the stage's output.
// c_4 is the carry of the next block.  The powers of M are made once per (row, stage) by repeated squaring.  No
// atomics, no workgroup waits on another, and nothing depends on where the row lies or on its neighbours: a row's
// output is bit-identical alone, packed at an odd offset, padded, in place, or beside rows with other stage counts.
// Contraction is off, so inside a piece the arithmetic is the restatement's own.
#include <math.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kThreads = 256;
constexpr int kLog2Piece = 4, kPiece = 1 << kLog2Piece;      // samples of one lane: 16 doubles in registers
constexpr int kBlock = kThreads * kPiece;                     // 4096 samples, 17 KB of LDS as padded float32
constexpr int kPad = kPiece + 1;                              // stride of the lanes' pieces in LDS: no bank conflict
constexpr int kMaxStages = 8;
constexpr int kPowers = 7;                                    // M^(2^j), j < 7: a wave's lanes, and M^64 between waves
constexpr int kWaves = kThreads / 64;
constexpr long kMaxSamples = (1L << 31) - 8;
constexpr double kMaxPoleRadius = 1.0 - 1.0 / 4096.0;         // 1 - 2^-12: the bound's amplification (1 - r)^-2 <= 2^24

struct Mat2 { double a, b, c, d; };                           // {{a, b}, {c, d}}

__device__ __forceinline__ Mat2 mat_mul(const Mat2& p, const Mat2& q) {
#pragma clang fp contract(off)
  return Mat2{p.a * q.a + p.b * q.c, p.a * q.b + p.b * q.d, p.c * q.a + p.d * q.c, p.c * q.b + p.d * q.d};
}

__global__ __launch_bounds__(kThreads) void augment_biquad_kernel(const float* x, const long* __restrict__ meta,
                                                                  int meta_fields, const double* __restrict__ sos,
                                                                  const int* __restrict__ n_stages, float* y) {
#pragma clang fp contract(off)
  __shared__ float s_x[kThreads * kPad];
  __shared__ double s_c[kMaxStages][5];
  __shared__ double s_pow[kMaxStages][kPowers][4];
  __shared__ double s_carry[kMaxStages][2];
  __shared__ double s_end[2][kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long* m = meta + (long)blockIdx.x * meta_fields;
  const long n = m[kRowLength];
  const float* xr = x + m[kRowOffset];
  float* yr = y + m[kRowOffset];
  int stages = n_stages[blockIdx.x];
  stages = stages < 0 ? 0 : (stages > kMaxStages ? kMaxStages : stages);
  if (tid < kMaxStages * 5) s_c[tid / 5][tid % 5] = sos[(long)blockIdx.x * kMaxStages * 5 + tid];
  if (tid < kMaxStages) { s_carry[tid][0] = 0.0; s_carry[tid][1] = 0.0; }
  __syncthreads();
  if (tid < stages) {
    Mat2 p{-s_c[tid][3], 1.0, -s_c[tid][4], 0.0};
    for (int j = 0; j < kLog2Piece; ++j) p = mat_mul(p, p);
    for (int j = 0; j < kPowers; ++j) {
      s_pow[tid][j][0] = p.a; s_pow[tid][j][1] = p.b; s_pow[tid][j][2] = p.c; s_pow[tid][j][3] = p.d;
      p = mat_mul(p, p);
    }
  }
  __syncthreads();
  int parity = 0;
  for (long c0 = 0; c0 < n; c0 += kBlock) {
    const int len = (int)(n - c0 < kBlock ? n - c0 : kBlock);
    for (int j = tid; j < kBlock; j += kThreads)
      s_x[(j >> kLog2Piece) * kPad + (j & (kPiece - 1))] = j < len ? xr[c0 + j] : 0.f;
    __syncthreads();
    double v[kPiece];
#pragma unroll
    for (int u = 0; u < kPiece; ++u) v[u] = (double)s_x[tid * kPad + u];
    for (int s = 0; s < stages; ++s) {
      const double b0 = s_c[s][0], b1 = s_c[s][1], b2 = s_c[s][2], a1 = s_c[s][3], a2 = s_c[s][4];
      double c1 = s_carry[s][0], c2 = s_carry[s][1];
      // 1. the piece from a zero state
      double e1 = 0.0, e2 = 0.0;
#pragma unroll
      for (int u = 0; u < kPiece; ++u) {
        const double o = b0 * v[u] + e1;
        e1 = b1 * v[u] - a1 * o + e2;
        e2 = b2 * v[u] - a2 * o;
      }
      // 2. the wave's scan, the wave ends in order, the lane's own start
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double o1 = __shfl_up(e1, 1u << j, 64), o2 = __shfl_up(e2, 1u << j, 64);
        const double* p = s_pow[s][j];
        if (lane >= (1 << j)) {
          e1 += p[0] * o1 + p[1] * o2;
          e2 += p[2] * o1 + p[3] * o2;
        }
      }
      double z1 = __shfl_up(e1, 1u, 64), z2 = __shfl_up(e2, 1u, 64);
      if (lane == 0) { z1 = 0.0; z2 = 0.0; }
      if (lane == 63) { s_end[parity][wave][0] = e1; s_end[parity][wave][1] = e2; }
      __syncthreads();
      {
        const double* p = s_pow[s][6];
        double w1 = c1, w2 = c2;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          if (w == wave) { c1 = w1; c2 = w2; }
          const double t1 = p[0] * w1 + p[1] * w2 + s_end[parity][w][0];
          const double t2 = p[2] * w1 + p[3] * w2 + s_end[parity][w][1];
          w1 = t1; w2 = t2;
        }
        if (tid == kThreads - 1) { s_carry[s][0] = w1; s_carry[s][1] = w2; }
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double* p = s_pow[s][j];
        if ((lane >> j) & 1) {
          const double t1 = p[0] * c1 + p[1] * c2, t2 = p[2] * c1 + p[3] * c2;
          c1 = t1; c2 = t2;
        }
      }
      z1 += c1; z2 += c2;
      // 3. the piece from its state
#pragma unroll
      for (int u = 0; u < kPiece; ++u) {
        const double o = b0 * v[u] + z1;
        z1 = b1 * v[u] - a1 * o + z2;
        z2 = b2 * v[u] - a2 * o;
        v[u] = o;
      }
      parity ^= 1;
    }
#pragma unroll
    for (int u = 0; u < kPiece; ++u) s_x[tid * kPad + u] = (float)v[u];
    __syncthreads();
    for (int j = tid; j < len; j += kThreads) yr[c0 + j] = s_x[(j >> kLog2Piece) * kPad + (j & (kPiece - 1))];
    __syncthreads();
  }
}

// y = float32(x g[row]): the gain and the polarity of a row in one multiply; g = 1 leaves the row's bits alone
__global__ __launch_bounds__(kThreads) void augment_gain_kernel(const float* x, const long* __restrict__ meta,
                                                                int meta_fields, const float* __restrict__ gains,
                                                                float* y) {
  const long* m = meta + (long)blockIdx.y * meta_fields;
  const long n = m[kRowLength];
  const float g = gains[blockIdx.y];
  const float* xr = x + m[kRowOffset];
  float* yr = y + m[kRowOffset];
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) yr[i] = xr[i] * g;
}

bool rows_ok(const long* host_meta, int meta_fields, int n_rows, long* samples, long* longest) {
  *samples = 0; *longest = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = host_meta + (long)r * meta_fields;
    if (m[kRowOffset] < 0 || m[kRowLength] < 0 || m[kRowLength] > kMaxSamples) return false;
    *samples += m[kRowLength];
    if (m[kRowLength] > *longest) *longest = m[kRowLength];
  }
  return true;
}

// {b0, b1, b2, a1, a2} finite, the poles inside the stability triangle and no further out than kMaxPoleRadius
bool stage_ok(const double* c) {
  for (int j = 0; j < 5; ++j)
    if (!isfinite(c[j])) return false;
  const double a1 = c[3], a2 = c[4];
  if (!(fabs(a2) < 1.0) || !(fabs(a1) < 1.0 + a2)) return false;
  const double disc = a1 * a1 - 4.0 * a2;
  const double radius = disc < 0.0 ? sqrt(a2) : 0.5 * (fabs(a1) + sqrt(disc));
  return radius <= kMaxPoleRadius;
}

}  // namespace

/* Host only; see include/pitchextractor_hip.h. */
extern "C" int pe_augment_biquad_consts(long* consts3) {
  if (!consts3) return PE_E_ARG;
  consts3[0] = kPiece; consts3[1] = kBlock; consts3[2] = kMaxStages;
  return PE_OK;
}

extern "C" int pe_augment_biquad(const float* x, const long* meta, const long* host_meta, int meta_fields, int n_rows,
                                 const double* sos, const double* host_sos, const int* n_stages,
                                 const int* host_n_stages, float* y, void* stream) {
  if (meta_fields < kRowHeader) return PE_E_ARG;
  long samples = 0, longest = 0;
  PE_OPEN(open_rows(n_rows, PE_OK, host_meta,
                    [&] { return rows_ok(host_meta, meta_fields, n_rows, &samples, &longest); }, nullptr));
  if (!host_sos || !host_n_stages) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    if (host_n_stages[r] < 0 || host_n_stages[r] > kMaxStages) return PE_E_ARG;
    for (int s = 0; s < host_n_stages[r]; ++s)
      if (!stage_ok(host_sos + ((long)r * kMaxStages + s) * 5)) return PE_E_ARG;
  }
  if (samples == 0) return PE_OK;
  if (!x || !meta || !sos || !n_stages || !y) return PE_E_ARG;
  hipLaunchKernelGGL(augment_biquad_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), x, meta, meta_fields,
                     sos, n_stages, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_augment_gain(const float* x, const long* meta, const long* host_meta, int meta_fields, int n_rows,
                               const float* gains, const float* host_gains, float* y, void* stream) {
  if (meta_fields < kRowHeader) return PE_E_ARG;
  long samples = 0, longest = 0;
  PE_OPEN(open_rows(n_rows, PE_OK, host_meta,
                    [&] { return rows_ok(host_meta, meta_fields, n_rows, &samples, &longest); }, nullptr));
  if (!host_gains) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (!isfinite(host_gains[r])) return PE_E_ARG;
  if (samples == 0) return PE_OK;
  if (!x || !meta || !gains || !y) return PE_E_ARG;
  const dim3 grid(grid_for(longest, 4 * kThreads, 64), n_rows);
  hipLaunchKernelGGL(augment_gain_kernel, grid, dim3(kThreads), 0, pe_stream(stream), x, meta, meta_fields, gains, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
