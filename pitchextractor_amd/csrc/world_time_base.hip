// The time base of WORLD's Synthesis (GetTimeBase + GetPulseLocationsForTimeBase) on ragged batches, with the phase as
// an exact integer: in turns of 2^-64 the per-sample increment f0i / fs is an unsigned 64-bit integer and the running
// sum a 128-bit one, whose low word is the wrapped phase and whose high word the number of pulses so far.  Integer
// addition is associative, so any piece size, scan order or batch layout gives the same bits; the definition and the
// Python-int restatement are tests/world_time_base_ref.py.
//
// pe_world_time_base_plan (host only) lays the rows out: the sample prefix, the samples n = int(L frame_period_ms fs /
// 1000), the frames L, the row's offset in the packed extended coarse curves (L + 1 doubles per row and curve), its
// pieces of kTbPiece samples counted from the row's own first sample and their prefix, the first pulse slot and the
// slot capacity floor(n max(cf_ext, 500) / fs) + 1.  Three launches, and no workgroup waits on another:
//   sums:    one workgroup per (row, piece): a thread forms the increments of its kTbRun samples, the workgroup adds
//            them to one 128-bit sum (wave shuffles, then the four waves in order).
//   scan:    one workgroup per row: the exclusive scan of the row's piece sums, 256 pieces per round; counts[row] is the
//            high word of the row's total.
//   pulses:  one workgroup per (row, piece): the increments again and the one past the piece's end, the inclusive
//            128-bit scan from the piece's prefix; the thread that owns sample i writes pulse hi_i where hi_(i+1) ==
//            hi_i + 1.  Every slot is written by exactly one thread; a slot at or beyond the row's capacity is not
//            written and sets the status word (it cannot happen with the plan's own meta).
// Everything per sample is double with contraction off (IEEE + - * /, floor, rint, compares and conversions), so a
// row's tables are the restatement's bit for bit, alone or anywhere in a batch.  No atomics, no spin loops.
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "dsp.h"

using namespace pe;

namespace {

constexpr int kTbThreads = 256;
constexpr int kTbRun = 16;                            // consecutive samples of one thread
constexpr int kTbPiece = kTbRun * kTbThreads;         // 4096 samples
constexpr long kTbMaxSamples = (1L << 31) - 8;
constexpr double kUnvoicedF0 = 500.0;
constexpr double kTwo64 = 18446744073709551616.0;

enum { T_SOFF, T_N, T_L, T_COFF, T_PIECES, T_POFF, T_SLOT, T_CAP, T_K };
static_assert(T_SOFF == kRowOffset && T_N == kRowLength, "the plan opens with the shared row header");
enum { TOT_PIECES, TOT_SLOTS, TOT_SAMPLES };
enum { STAGE_SUMS = 1, STAGE_SCAN = 2, STAGE_PULSES = 4, STAGE_ALL = 7 };

struct U128 {
  uint64_t lo, hi;
};

__host__ __device__ __forceinline__ U128 add128(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < b.lo ? 1ULL : 0ULL);
  return r;
}

bool config_ok(double fs, double frame_period_ms) {
  return isfinite(fs) && fs > 0.0 && isfinite(frame_period_ms) && frame_period_ms > 0.0 && kUnvoicedF0 < fs / 2.0;
}

bool meta_ok(const long* hm, int n_rows, double fs, double frame_period_ms, long* totals3) {
  long s = 0, p = 0, c = 0, q = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long* m = hm + (long)r * T_K;
    if (m[T_L] < 2 || m[T_L] > kTbMaxSamples) return false;
    const double nd = ((double)m[T_L] * frame_period_ms) * fs / 1000.0;
    if (!(nd < (double)kTbMaxSamples) || m[T_N] != (long)nd) return false;
    if (m[T_SOFF] != s || m[T_COFF] != c || m[T_POFF] != p || m[T_SLOT] != q) return false;
    if (m[T_PIECES] != (m[T_N] + kTbPiece - 1) / kTbPiece) return false;
    if (m[T_CAP] < 1 || m[T_CAP] > m[T_N] / 2 + 1) return false;      // every value is below fs / 2
    s += m[T_N]; p += m[T_PIECES]; c += m[T_L] + 1; q += m[T_CAP];
  }
  totals3[TOT_PIECES] = p; totals3[TOT_SLOTS] = q; totals3[TOT_SAMPLES] = s;
  return true;
}

// Sample i of a row: the voicing and the interpolated F0 of the definition, and the increment rint(f0i / fs 2^64).
// cf / cv: the row's extended coarse curves (L + 1 values), ct[j] = j fp.
__device__ __forceinline__ uint64_t sample_inc(const double* __restrict__ cf, const double* __restrict__ cv, long L,
                                               double fp, double fs, long i, bool& voiced, double& f0i) {
#pragma clang fp contract(off)
  const double t = (double)i / fs;
  const double q = floor(t / fp);
  long j = q < 0.0 ? 0 : (q > (double)(L - 1) ? L - 1 : (long)q);
  for (int it = 0; it < 4 && j > 0 && (double)j * fp > t; ++it) --j;
  for (int it = 0; it < 4 && j < L - 1 && (double)(j + 1) * fp <= t; ++it) ++j;
  const double x0 = (double)j * fp, x1 = (double)(j + 1) * fp;
  const double dt = t - x0, dx = x1 - x0;
  const double v = ((cv[j + 1] - cv[j]) / dx) * dt + cv[j];
  voiced = v > 0.5;
  f0i = voiced ? ((cf[j + 1] - cf[j]) / dx) * dt + cf[j] : kUnvoicedF0;
  return (uint64_t)rint((f0i / fs) * kTwo64);
}

__device__ __forceinline__ U128 shfl_xor128(U128 v, int off) {
  U128 o;
  o.lo = (uint64_t)__shfl_xor((unsigned long long)v.lo, off, 64);
  o.hi = (uint64_t)__shfl_xor((unsigned long long)v.hi, off, 64);
  return o;
}

// The sum of one U128 per thread over the workgroup; every thread gets it.  s_w: 4 U128.
__device__ __forceinline__ U128 block_sum128(U128 v, U128* s_w, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = add128(v, shfl_xor128(v, off));
  __syncthreads();
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  return add128(add128(s_w[0], s_w[1]), add128(s_w[2], s_w[3]));
}

// The sum of the threads before `tid`, and the sum of all in `total`.  s_w: 4 U128.
__device__ __forceinline__ U128 block_scan128(U128 v, U128* s_w, int tid, U128& total) {
  const int lane = tid & 63, wave = tid >> 6;
  U128 inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    U128 o;
    o.lo = (uint64_t)__shfl_up((unsigned long long)inc.lo, off, 64);
    o.hi = (uint64_t)__shfl_up((unsigned long long)inc.hi, off, 64);
    if (lane >= off) inc = add128(inc, o);
  }
  U128 prev;
  prev.lo = (uint64_t)__shfl_up((unsigned long long)inc.lo, 1, 64);
  prev.hi = (uint64_t)__shfl_up((unsigned long long)inc.hi, 1, 64);
  if (lane == 0) prev = U128{0, 0};
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  U128 before = prev, all = U128{0, 0};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before = add128(before, s_w[w]);
    all = add128(all, s_w[w]);
  }
  total = all;
  return before;
}

__global__ __launch_bounds__(kTbThreads) void time_base_sums_kernel(const long* __restrict__ meta,
                                                                    const double* __restrict__ cf_ext,
                                                                    const double* __restrict__ cv_ext, int n_rows,
                                                                    long pieces, double fs, double fp,
                                                                    U128* __restrict__ sums) {
  __shared__ U128 s_w[4];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, T_K, T_POFF, g);
    const long* m = meta + (long)row * T_K;
    const long n = m[T_N], L = m[T_L], i0 = (g - m[T_POFF]) * kTbPiece + (long)tid * kTbRun;
    const double* cf = cf_ext + m[T_COFF];
    const double* cv = cv_ext + m[T_COFF];
    U128 local{0, 0};
#pragma unroll 4
    for (int u = 0; u < kTbRun; ++u) {
      if (i0 + u < n) {
        bool voiced;
        double f0i;
        local = add128(local, U128{sample_inc(cf, cv, L, fp, fs, i0 + u, voiced, f0i), 0});
      }
    }
    const U128 total = block_sum128(local, s_w, tid);
    if (tid == 0) sums[g] = total;
  }
}

// sums[piece prefix + k] -> the sum of the row's pieces before k; counts[row] = the high word of the row's total
__global__ __launch_bounds__(kTbThreads) void time_base_scan_kernel(const long* __restrict__ meta,
                                                                    U128* __restrict__ sums,
                                                                    long* __restrict__ counts) {
  __shared__ U128 s_w[4];
  const int tid = threadIdx.x;
  const long* m = meta + (long)blockIdx.x * T_K;
  const long pieces = m[T_PIECES];
  U128* s = sums + m[T_POFF];
  U128 carry{0, 0};
  for (long base = 0; base < pieces; base += kTbThreads) {          // uniform over the workgroup
    const long k = base + tid;
    const U128 v = k < pieces ? s[k] : U128{0, 0};
    U128 total;
    const U128 before = block_scan128(v, s_w, tid, total);
    if (k < pieces) s[k] = add128(carry, before);
    carry = add128(carry, total);
  }
  if (tid == 0) counts[blockIdx.x] = (long)carry.hi;
}

__global__ __launch_bounds__(kTbThreads) void time_base_pulses_kernel(
    const long* __restrict__ meta, const double* __restrict__ cf_ext, const double* __restrict__ cv_ext, int n_rows,
    long pieces, double fs, double fp, const U128* __restrict__ sums, long* __restrict__ index,
    double* __restrict__ shift, unsigned char* __restrict__ vuv, int* __restrict__ status, double* __restrict__ hook_f0i,
    uint64_t* __restrict__ hook_lo, long* __restrict__ hook_hi) {
#pragma clang fp contract(off)
  __shared__ U128 s_w[4];
  const int tid = threadIdx.x;
  for (long g = blockIdx.x; g < pieces; g += gridDim.x) {
    const int row = find_row(meta, n_rows, T_K, T_POFF, g);
    const long* m = meta + (long)row * T_K;
    const long n = m[T_N], L = m[T_L], i0 = (g - m[T_POFF]) * kTbPiece + (long)tid * kTbRun;
    const long soff = m[T_SOFF], slot0 = m[T_SLOT], cap = m[T_CAP];
    const double* cf = cf_ext + m[T_COFF];
    const double* cv = cv_ext + m[T_COFF];
    uint64_t inc[kTbRun + 1];
    unsigned voiced_bits = 0;
    U128 local{0, 0};
#pragma unroll
    for (int u = 0; u <= kTbRun; ++u) {                              // the last one belongs to the next thread or piece
      inc[u] = 0;
      if (i0 + u < n) {
        bool voiced;
        double f0i;
        inc[u] = sample_inc(cf, cv, L, fp, fs, i0 + u, voiced, f0i);
        if (voiced) voiced_bits |= 1u << u;
        if (u < kTbRun && hook_f0i) hook_f0i[soff + i0 + u] = f0i;
      }
      if (u < kTbRun) local = add128(local, U128{inc[u], 0});
    }
    U128 total;
    U128 run = add128(sums[g], block_scan128(local, s_w, tid, total));
#pragma unroll
    for (int u = 0; u < kTbRun; ++u) {
      const long i = i0 + u;
      if (i < n) {
        run = add128(run, U128{inc[u], 0});
        if (hook_lo) hook_lo[soff + i] = run.lo;
        if (hook_hi) hook_hi[soff + i] = (long)run.hi;
        if (i + 1 < n && run.lo + inc[u + 1] < run.lo) {             // hi_(i+1) == hi_i + 1: pulse number hi_i
          const long p = (long)run.hi;
          if (p >= 0 && p < cap) {
            const double rest = run.lo == 0 ? kTwo64 : (double)(0ULL - run.lo);
            const double x = rest / (double)inc[u + 1];
            index[slot0 + p] = i;
            shift[slot0 + p] = x / fs;
            vuv[slot0 + p] = (voiced_bits >> u) & 1u;
          } else {
            *status = 1;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int pe_world_time_base_plan_fields(void) { return T_K; }

/* Host-only layout; see include/pitchextractor_hip.h. */
extern "C" int pe_world_time_base_plan(int n_rows, const long* n_frames, const double* cf_ext, const double* cv_ext,
                                       double fs, double frame_period_ms, long* meta, long* totals) {
  if (!totals || n_rows < 0 || n_rows > kMaxRows || !config_ok(fs, frame_period_ms)) return PE_E_ARG;
  if (n_rows > 0 && (!n_frames || !cf_ext || !cv_ext || !meta)) return PE_E_ARG;
  long s = 0, p = 0, c = 0, q = 0;
  for (int r = 0; r < n_rows; ++r) {
    const long L = n_frames[r];
    if (L < 2 || L > kTbMaxSamples) return PE_E_ARG;
    const double nd = ((double)L * frame_period_ms) * fs / 1000.0;
    if (!(nd < (double)kTbMaxSamples)) return PE_E_ARG;
    const long n = (long)nd;
    double top = kUnvoicedF0;
    for (long j = 0; j <= L; ++j) {
      const double f = cf_ext[c + j], v = cv_ext[c + j];
      if (!isfinite(f) || !isfinite(v) || f < 0.0 || !(f < fs / 2.0)) return PE_E_ARG;
      if (f > top) top = f;
    }
    long* m = meta + (long)r * T_K;
    m[T_SOFF] = s; m[T_N] = n; m[T_L] = L; m[T_COFF] = c; m[T_PIECES] = (n + kTbPiece - 1) / kTbPiece; m[T_POFF] = p;
    m[T_SLOT] = q; m[T_CAP] = (long)floor((double)n * top / fs) + 1;
    s += n; p += m[T_PIECES]; c += L + 1; q += m[T_CAP];
  }
  totals[TOT_PIECES] = p; totals[TOT_SLOTS] = q; totals[TOT_SAMPLES] = s;
  return PE_OK;
}

extern "C" size_t pe_world_time_base_workspace_bytes(long pieces) {
  return pieces > 0 ? (size_t)pieces * sizeof(U128) : 0;
}

extern "C" int pe_world_time_base(const double* cf_ext, const double* cv_ext, const long* meta, const long* host_meta,
                                  int n_rows, double fs, double frame_period_ms, int stages, long* index, double* shift,
                                  unsigned char* vuv, long* counts, int* status, double* f0i, unsigned long* lo,
                                  long* hi, void* workspace, size_t workspace_bytes, void* stream) {
  long tot[3] = {0, 0, 0};
  PE_OPEN(open_rows(n_rows, config_ok(fs, frame_period_ms) ? PE_OK : PE_E_ARG, host_meta,
                    [&] { return meta_ok(host_meta, n_rows, fs, frame_period_ms, tot); }, nullptr));
  if (stages < 1 || stages > STAGE_ALL) return PE_E_ARG;
  if (!cf_ext || !cv_ext || !meta || !index || !shift || !vuv || !counts || !status) return PE_E_ARG;
  const long pieces = tot[TOT_PIECES];
  if (pieces > 0 && (!workspace || workspace_bytes < pe_world_time_base_workspace_bytes(pieces))) return PE_E_WORKSPACE;
  U128* sums = static_cast<U128*>(workspace);
  const double fp = frame_period_ms / 1000.0;
  const dim3 grid(grid_of(pieces)), wg(kTbThreads);
  if ((stages & STAGE_SUMS) && pieces > 0) {
    hipLaunchKernelGGL(time_base_sums_kernel, grid, wg, 0, pe_stream(stream), meta, cf_ext, cv_ext, n_rows, pieces, fs,
                       fp, sums);
    PE_LAUNCH_CHECK();
  }
  if (stages & STAGE_SCAN) {                                         // rows without a sample get their count of 0 here
    hipLaunchKernelGGL(time_base_scan_kernel, dim3(n_rows), wg, 0, pe_stream(stream), meta, sums, counts);
    PE_LAUNCH_CHECK();
  }
  if ((stages & STAGE_PULSES) && pieces > 0) {
    hipLaunchKernelGGL(time_base_pulses_kernel, grid, wg, 0, pe_stream(stream), meta, cf_ext, cv_ext, n_rows, pieces,
                       fs, fp, sums, index, shift, vuv, status, f0i, reinterpret_cast<uint64_t*>(lo), hi);
    PE_LAUNCH_CHECK();
  }
  return PE_OK;
}
