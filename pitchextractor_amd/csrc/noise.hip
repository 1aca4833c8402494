// Additive noise at an SNR on ragged batches (the robustness curve the reference's
// Utils/noise_robustness_evaluation.ipynb is meant to draw): seeded standard normals, white noise coloured by a bank
// of one-pole sections, a recorded bed looped, and the mix at a signal-to-noise ratio with the notebooks' peak rule.
// Pinned by the float64 restatement in tests/noise_ref.py.
//
// pe_noise_plan (host only) lays the rows out: offset and length (the shared row header), the warm-up, the generated
// samples warm-up + n, the row's pieces of kPiece generated samples counted from the row's own first generated sample
// and their prefix, the seed and the offset of a given white input; and one table of doubles with the colour: d0, d1,
// the section count, and per section a, b and the powers of a the scan multiplies by, each made once on the host.
// Every stage is a fixed number of launches whatever the rows:
//   white:  y[i] = world_randn(seed, warm-up + i).  One.
//   colour: y[j] = d0 w[j] + d1 w[j - 1] + sum_k s_k[j], s_k[j] = a_k s_k[j - 1] + b_k w[j], over the generated
//           samples, of which the last n are written.  Piece end states from a zero state (a thread runs its kRun
//           samples, the threads are scanned as affine maps of equal length: s[t] += a^(kRun 2^m) s[t - 2^m]), carries
//           (per row one thread per section walks the row's pieces in order, carry' = a^kPiece carry + end), then the
//           piece scan again with thread 0 started from the carry, each thread running its samples from the state
//           before it.  Three, and no workgroup waits on another.
//   bed:    y[i] = bed[(start + i) mod L].  One.
//   mix:    the mix at an SNR of snr_mix.h (piece sums of squares, row rms and scale, y = x + float32(noise scale)
//           and piece peaks, row peak, normalisation), which pe_stim_finish runs too.  Five, four without the peak
//           rule: a row here may have thousands of pieces, so the row peaks take a launch of their own.
// Sums and recurrences are double with contraction off; nothing a row computes depends on where the row lies or on
// its neighbours: a row's result is the same alone, packed at an odd offset or padded.
#include <math.h>
#include "common.h"
#include "snr_mix.h"

using namespace pe;

namespace {

constexpr int kSteps = 8;                        // scan steps over the threads: 2^kSteps == kThreads
constexpr int kMaxSections = 8;
constexpr long kMaxSamples = (1L << 31) - 8;

enum { N_OFF, N_N, N_WARM, N_GEN, N_PIECES, N_POFF, N_SEED, N_WOFF, N_K };
static_assert(N_OFF == kRowOffset && N_N == kRowLength, "the plan opens with the shared row header");
enum { TOT_SAMPLES, TOT_PIECES };
// the colour: d0, d1, sections, -, then per section {a, b, a^(kRun 2^m) for m < kSteps, a^kPiece, -}
enum { C_D0, C_D1, C_NSEC, C_SPARE, C_SECTIONS };
enum { Q_A, Q_B, Q_POW, Q_PIECE = Q_POW + kSteps, Q_SPARE, Q_K };
constexpr int C_K = C_SECTIONS + kMaxSections * Q_K;
enum { B_OFF, B_LEN, B_START, B_K };             // a row's bed: offset in the bed audio, length, first sample

// The plan as snr_mix.h reads it: x -> y without a fade, the noise where the row lies, one snr_db per row in an array;
// a row may have thousands of pieces.  (The plan's pieces count the generated samples, the mix's the row's n.)
struct NoiseMixRows {
  static constexpr int kFields = N_K, kPieceOffset = N_POFF, kFade = -1, kNoiseOffset = -1, kSnrStride = 1;
  static constexpr bool kInPlace = false, kPeakLaunch = true;
};

long pieces_of(long n, long gen) { return n > 0 ? (gen + kPiece - 1) / kPiece : 0; }

bool meta_ok(const long* hm, int n_rows, long* totals2) {
  long s = 0, p = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * N_K;
    if (m[N_N] < 0 || m[N_N] > kMaxSamples || m[N_OFF] < 0 || m[N_WARM] < 0 || m[N_WARM] > kMaxSamples) return false;
    if (m[N_GEN] != m[N_N] + m[N_WARM] || m[N_GEN] > kMaxSamples || m[N_WOFF] < -1) return false;
    if (m[N_PIECES] != pieces_of(m[N_N], m[N_GEN]) || m[N_POFF] != p) return false;
    s += m[N_N]; p += m[N_PIECES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_PIECES] = p;
  return true;
}

int open_batch(int n_rows, const long* host_meta, long* totals2) {
  return open_rows(n_rows, PE_OK, host_meta, [&] { return meta_ok(host_meta, n_rows, totals2); },
                   &totals2[TOT_SAMPLES]);
}

// The colour table of {d0, d1, (a, b) per section}: false for more than kMaxSections sections, a non-finite
// coefficient or a pole on or outside the unit circle.  The powers by repeated multiplication and squaring.
bool fill_colour(const double* coeffs, int n_sections, double* prm) {
#pragma clang fp contract(off)
  if (n_sections < 0 || n_sections > kMaxSections || !coeffs) return false;
  for (int j = 0; j < C_K; ++j) prm[j] = 0.0;
  if (!isfinite(coeffs[0]) || !isfinite(coeffs[1])) return false;
  prm[C_D0] = coeffs[0]; prm[C_D1] = coeffs[1]; prm[C_NSEC] = (double)n_sections;
  for (int k = 0; k < n_sections; ++k) {
    const double a = coeffs[2 + 2 * k], b = coeffs[3 + 2 * k];
    if (!isfinite(a) || !isfinite(b) || !(fabs(a) < 1.0)) return false;
    double* q = prm + C_SECTIONS + k * Q_K;
    q[Q_A] = a; q[Q_B] = b;
    double pw = a;
    for (int u = 1; u < kRun; ++u) pw *= a;
    for (int m = 0; m < kSteps; ++m) { q[Q_POW + m] = pw; pw *= pw; }
    q[Q_PIECE] = pw;
  }
  return true;
}

// a host table that fill_colour made
bool colour_ok(const double* hp) {
  if (!hp || !(hp[C_NSEC] >= 0.0 && hp[C_NSEC] <= (double)kMaxSections) || hp[C_NSEC] != floor(hp[C_NSEC])) return false;
  const int n_sections = (int)hp[C_NSEC];
  double coeffs[2 + 2 * kMaxSections], again[C_K];
  coeffs[0] = hp[C_D0]; coeffs[1] = hp[C_D1];
  for (int k = 0; k < n_sections; ++k) {
    coeffs[2 + 2 * k] = hp[C_SECTIONS + k * Q_K + Q_A];
    coeffs[3 + 2 * k] = hp[C_SECTIONS + k * Q_K + Q_B];
  }
  if (!fill_colour(coeffs, n_sections, again)) return false;
  return memcmp(again, hp, sizeof(again)) == 0;
}

// ---- white ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void noise_white_kernel(const long* __restrict__ meta, int n_rows, long pieces,
                                                               float* __restrict__ y) {
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, N_K, N_POFF, g);
    const long* m = meta + (long)row * N_K;
    const long n = m[N_N], warm = m[N_WARM], base = (g - m[N_POFF]) * kPiece;
    const uint64_t seed = (uint64_t)m[N_SEED];
    float* out = y + m[N_OFF];
    for (int j = tid; j < kPiece && base + j < n; j += kThreads)
      out[base + j] = world_randn(seed, (uint64_t)(warm + base + j));
  }
}

// ---- colour --------------------------------------------------------------------------------------------------------
// Piece g of a row: thread t owns generated samples [t kRun, (t + 1) kRun) of the piece, zero beyond the row's last.
// WRITE == false: ends[g][k] = the state of section k after the piece, from a zero state.  WRITE == true: ends[g][k]
// holds the state before the piece; y[j - warm-up] = float32(d0 w[j] + d1 w[j - 1] + sum_k s_k[j]) for j >= warm-up.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void noise_colour_kernel(const long* __restrict__ meta,
                                                                const double* __restrict__ prm,
                                                                const float* __restrict__ white, int n_rows,
                                                                long pieces, double* __restrict__ ends,
                                                                float* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ double s_st[kMaxSections][kThreads];
  const int tid = threadIdx.x;
  const int nsec = (int)prm[C_NSEC];
  double a[kMaxSections], b[kMaxSections];
#pragma unroll
  for (int k = 0; k < kMaxSections; ++k) {
    a[k] = k < nsec ? prm[C_SECTIONS + k * Q_K + Q_A] : 0.0;
    b[k] = k < nsec ? prm[C_SECTIONS + k * Q_K + Q_B] : 0.0;
  }
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, N_K, N_POFF, g);
    const long* m = meta + (long)row * N_K;
    const long gen = m[N_GEN], warm = m[N_WARM], j0 = (g - m[N_POFF]) * kPiece + (long)tid * kRun;
    const uint64_t seed = (uint64_t)m[N_SEED];
    const float* wr = white && m[N_WOFF] >= 0 ? white + m[N_WOFF] : nullptr;
    auto w_at = [&](long j) { return (double)(wr ? wr[j] : world_randn(seed, (uint64_t)j)); };
    double w[kRun];
#pragma unroll
    for (int u = 0; u < kRun; ++u) w[u] = j0 + u < gen ? w_at(j0 + u) : 0.0;
    // the thread's run from a zero state (thread 0 of the second pass: from the state before the piece)
#pragma unroll
    for (int k = 0; k < kMaxSections; ++k)
      if (k < nsec) {
        double st = WRITE && tid == 0 ? ends[g * kMaxSections + k] : 0.0;
#pragma unroll
        for (int u = 0; u < kRun; ++u) st = a[k] * st + b[k] * w[u];
        s_st[k][tid] = st;
      }
    __syncthreads();
    for (int step = 0; step < kSteps; ++step) {
      const int back = 1 << step;
      double add[kMaxSections];
#pragma unroll
      for (int k = 0; k < kMaxSections; ++k)
        add[k] = k < nsec && tid >= back ? prm[C_SECTIONS + k * Q_K + Q_POW + step] * s_st[k][tid - back] : 0.0;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kMaxSections; ++k)
        if (k < nsec && tid >= back) s_st[k][tid] += add[k];
      __syncthreads();
    }
    if (!WRITE) {
      if (tid < nsec) ends[g * kMaxSections + tid] = s_st[tid][kThreads - 1];
    } else {
      double st[kMaxSections];
#pragma unroll
      for (int k = 0; k < kMaxSections; ++k)
        st[k] = k < nsec ? (tid > 0 ? s_st[k][tid - 1] : ends[g * kMaxSections + k]) : 0.0;
      const double d0 = prm[C_D0], d1 = prm[C_D1];
      double before = j0 > 0 && j0 - 1 < gen ? w_at(j0 - 1) : 0.0;
      float* out = y + m[N_OFF];
#pragma unroll
      for (int u = 0; u < kRun; ++u) {
        double acc = d0 * w[u] + d1 * before;
#pragma unroll
        for (int k = 0; k < kMaxSections; ++k)
          if (k < nsec) {
            st[k] = a[k] * st[k] + b[k] * w[u];
            acc += st[k];
          }
        const long j = j0 + u;
        if (j >= warm && j < gen) out[j - warm] = (float)acc;
        before = w[u];
      }
    }
    __syncthreads();
  }
}

// ends[piece prefix + p][k] -> the state of section k before piece p.  One workgroup per row: kThreads pieces at a time
// come into LDS with every thread loading, thread k walks section k through them in piece order, and they go back.
__global__ __launch_bounds__(kThreads) void noise_carry_kernel(const long* __restrict__ meta,
                                                               const double* __restrict__ prm,
                                                               double* __restrict__ ends) {
#pragma clang fp contract(off)
  __shared__ double s_e[kThreads * kMaxSections];
  const int tid = threadIdx.x, nsec = (int)prm[C_NSEC];
  const long* m = meta + (long)blockIdx.x * N_K;
  const long pieces = m[N_PIECES];
  const double ap = tid < nsec ? prm[C_SECTIONS + tid * Q_K + Q_PIECE] : 0.0;
  double* e = ends + m[N_POFF] * kMaxSections;
  double carry = 0.0;
  for (long p0 = 0; p0 < pieces; p0 += kThreads) {
    const int count = (int)(pieces - p0 < kThreads ? pieces - p0 : kThreads);
    for (int i = tid; i < count * kMaxSections; i += kThreads) s_e[i] = e[p0 * kMaxSections + i];
    __syncthreads();
    if (tid < nsec)
      for (int p = 0; p < count; ++p) {
        const double v = s_e[p * kMaxSections + tid];
        s_e[p * kMaxSections + tid] = carry;
        carry = ap * carry + v;
      }
    __syncthreads();
    for (int i = tid; i < count * kMaxSections; i += kThreads) e[p0 * kMaxSections + i] = s_e[i];
    __syncthreads();
  }
}

// ---- bed -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void noise_bed_kernel(const long* __restrict__ meta,
                                                             const float* __restrict__ bed,
                                                             const long* __restrict__ beds, int n_rows, long pieces,
                                                             float* __restrict__ y) {
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, N_K, N_POFF, g);
    const long* m = meta + (long)row * N_K;
    const long* bd = beds + (long)row * B_K;
    const long n = m[N_N], base = (g - m[N_POFF]) * kPiece, L = bd[B_LEN];
    const float* src = bed + bd[B_OFF];
    float* out = y + m[N_OFF];
    long at = (bd[B_START] + base + tid) % L;           // then kThreads further each time, wrapped without a division
    const long step = kThreads % L;
    for (int j = tid; j < kPiece && base + j < n; j += kThreads) {
      out[base + j] = src[at];
      at += step;
      if (at >= L) at -= L;
    }
  }
}

}  // namespace

extern "C" int pe_noise_plan_fields(void) { return N_K; }
extern "C" int pe_noise_param_fields(void) { return C_K; }

/* Host-only layout and colour table; see include/pitchextractor_hip.h. */
extern "C" int pe_noise_plan(int n_rows, const long* n, const long* y_off, const long* warmup, const long* seeds,
                             const long* white_off, const double* coeffs, int n_sections, long* consts4, long* meta,
                             double* params, long* totals2) {
  if (!consts4 || !totals2 || !params || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows > 0 && (!n || !y_off || !warmup || !seeds || !white_off || !meta)) return PE_E_ARG;
  consts4[0] = kPiece; consts4[1] = kMaxSections; consts4[2] = ST_K; consts4[3] = B_K;
  if (!fill_colour(coeffs, n_sections, params)) return PE_E_ARG;
  long s = 0, pc = 0;
  for (int r = 0; r < n_rows; ++r) {
    if (n[r] < 0 || n[r] > kMaxSamples || y_off[r] < 0 || warmup[r] < 0 || warmup[r] > kMaxSamples) return PE_E_ARG;
    if (n[r] + warmup[r] > kMaxSamples || white_off[r] < -1) return PE_E_ARG;
    long* m = meta + (long)r * N_K;
    m[N_OFF] = y_off[r]; m[N_N] = n[r]; m[N_WARM] = warmup[r]; m[N_GEN] = n[r] + warmup[r];
    m[N_PIECES] = pieces_of(m[N_N], m[N_GEN]); m[N_POFF] = pc; m[N_SEED] = seeds[r]; m[N_WOFF] = white_off[r];
    s += n[r]; pc += m[N_PIECES];
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_PIECES] = pc;
  return PE_OK;
}

extern "C" size_t pe_noise_workspace_bytes(long pieces) {
  return pieces > 0 ? (size_t)pieces * kMaxSections * sizeof(double) : 0;
}

extern "C" int pe_noise_white(const long* meta, const long* host_meta, int n_rows, float* y, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!meta || !y) return PE_E_ARG;
  hipLaunchKernelGGL(noise_white_kernel, dim3(grid_of(tot[TOT_PIECES])), dim3(kThreads), 0, pe_stream(stream), meta,
                     n_rows, tot[TOT_PIECES], y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_noise_colour(const long* meta, const long* host_meta, const double* params,
                               const double* host_params, const float* white, long n_white, int n_rows, float* y,
                               void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2];
  PE_OPEN(open_rows(n_rows, colour_ok(host_params) ? PE_OK : PE_E_ARG, host_meta,
                    [&] { return meta_ok(host_meta, n_rows, tot); }, &tot[TOT_SAMPLES]));
  for (int r = 0; r < n_rows; ++r) {                   // a given white input covers the row's generated samples
    const long* m = host_meta + (long)r * N_K;
    if (m[N_WOFF] >= 0 && (!white || m[N_WOFF] + m[N_GEN] > n_white)) return PE_E_ARG;
  }
  if (!meta || !params || !y) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_noise_workspace_bytes(tot[TOT_PIECES])) return PE_E_WORKSPACE;
  double* ends = static_cast<double*>(workspace);
  const long pieces = tot[TOT_PIECES];
  const dim3 grid(grid_of(pieces)), wg(kThreads);
  hipLaunchKernelGGL(noise_colour_kernel<false>, grid, wg, 0, pe_stream(stream), meta, params, white, n_rows, pieces,
                     ends, y);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(noise_carry_kernel, dim3(n_rows), wg, 0, pe_stream(stream), meta, params, ends);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(noise_colour_kernel<true>, grid, wg, 0, pe_stream(stream), meta, params, white, n_rows, pieces,
                     ends, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_noise_bed(const long* meta, const long* host_meta, const float* bed, long n_bed, const long* beds,
                            const long* host_beds, int n_rows, float* y, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!host_beds) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    const long* bd = host_beds + (long)r * B_K;
    if (bd[B_LEN] < 1 || bd[B_START] < 0 || bd[B_START] >= bd[B_LEN] || bd[B_OFF] < 0 || bd[B_LEN] > n_bed ||
        bd[B_OFF] > n_bed - bd[B_LEN])
      return PE_E_ARG;
  }
  if (!meta || !bed || !beds || !y) return PE_E_ARG;
  hipLaunchKernelGGL(noise_bed_kernel, dim3(grid_of(tot[TOT_PIECES])), dim3(kThreads), 0, pe_stream(stream), meta,
                     bed, beds, n_rows, tot[TOT_PIECES], y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_noise_mix(const float* x, const float* noise, const long* meta, const long* host_meta,
                            const double* snr_db, const double* host_snr_db, int peak_normalize, int n_rows, float* y,
                            double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  long tot[2];
  PE_OPEN(open_batch(n_rows, host_meta, tot));
  if (!host_snr_db) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (!isfinite(host_snr_db[r])) return PE_E_ARG;
  if (!x || !noise || !meta || !snr_db || !y || !stats) return PE_E_ARG;
  if (!workspace || workspace_bytes < pe_noise_workspace_bytes(tot[TOT_PIECES])) return PE_E_WORKSPACE;
  return launch_snr_mix<NoiseMixRows>(meta, n_rows, snr_db, tot[TOT_PIECES], x, noise, y, peak_normalize != 0, stats,
                                      static_cast<double*>(workspace), pe_stream(stream));
}
