// What the audio kernels (mel.hip, pitch_shift.hip, f0_track.hip, f0_dio.hip, world_synth.hip, cheaptrick.hip, d4c.hip,
// stress.hip, augment.hip, rir_synth.hip, stimuli.hip, noise.hip) share; on top of this, pieces.h holds what the last
// three share among themselves (the piece geometry, the double reductions and scan), snr_mix.h the mix at an SNR of the
// last two, and world_frames.h what the WORLD analyses cheaptrick.hip and d4c.hip share (the frame plan, the DC
// correction, the interval mean). Host: the row bound and the launch-grid clamps of the ragged entry points, the header
// every row plan opens with, the gate every entry point that takes a host plan passes before its own checks (open_rows,
// kNothing, PE_OPEN), the size of the transform roots every table opens with, and with_log2 (transform size -> kernel
// instance).  Device:
// float2 complex arithmetic, the wave-private LDS fence, the in-place radix-4 Stockham FFT in LDS, a packed half-length
// transform's bins as the real one's and back (real_fft_split, real_fft_bin, real_fft_pack), the 256-thread workgroup
// float reductions in a fixed order, the seeded standard normal (world_randn), and the row search of ragged plans.
#pragma once
#include <type_traits>
#include "common.h"

namespace pe {

constexpr int kMaxRows = 65535;           // rows of one ragged batch (a launch grid's y / x extent)
constexpr float kPiF = 3.14159265358979323846f;
// workgroups of a grid-stride launch: one per `per_block` work items, `cap` at the most
inline int grid_for(long work, int per_block, int cap) {
  const long b = (work + per_block - 1) / per_block;
  return (int)(b < cap ? b : cap);
}
inline unsigned grid_of(long items) { return (unsigned)grid_for(items, 1, 1 << 20); }
// floats of the roots every LDS-FFT table opens with: C float2 of the packed C-point transform (fft_lds's `tw`), then
// C + 1 float2 of its split into the real 2C-point one (`tr` of real_fft_bin)
constexpr long fft_table_floats(long C) { return 2 * C + 2 * (C + 1); }

// Every row plan (n_rows x K int64, K the plan's own field count) opens with the row's offset in `x` and its length in
// samples.  A plan's enum static_asserts this; what reads only this header (pe_row_stats) serves any plan given its K.
enum { kRowOffset = 0, kRowLength = 1, kRowHeader = 2 };

// The gate of an entry point that takes a ragged plan's host copy, in this order: n_rows outside [0, kMaxRows] is
// PE_E_ARG; `config` (the status of the plan's derive(sr, hop, config), PE_OK where there is none) is returned if it is
// an error, a bad one with no rows included; no rows is kNothing; a null host_meta, or one that consistent() (the plan's
// own walk over it, which also fills the totals) refuses, is PE_E_ARG; *work == 0 (the total a launch needs; null: none)
// is kNothing; else PE_OK, and the entry point's own pointer and size checks follow.  That is the order of the answers,
// not of evaluation: a caller's derive() has run, as an argument, before the range check, so it must be free of side
// effects and safe on null.  An entry point with host checks of its own between the plan and the work total
// (pe_stress_rir, pe_stress_agc) takes the status and answers kNothing itself after them.
constexpr int kNothing = 1;               // valid, and nothing to launch: PE_OK to the caller
template <class Consistent>
int open_rows(int n_rows, int config, const long* host_meta, Consistent&& consistent, const long* work) {
  if (n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (config != PE_OK) return config;
  if (n_rows == 0) return kNothing;
  if (!host_meta || !consistent()) return PE_E_ARG;
  return work && *work == 0 ? kNothing : PE_OK;
}
// leaves the entry point unless the gate says go
#define PE_OPEN(gate)                                           \
  do {                                                          \
    const int pe_st_ = (gate);                                  \
    if (pe_st_ != PE_OK) return pe_st_ == kNothing ? PE_OK : pe_st_; \
  } while (0)

// Calls fn(std::integral_constant<int, L>{}) for L == lg in [LO, HI] and returns its status; PE_E_UNSUPPORTED outside the
// range (what with_form of forms.h is for product forms).  The one other fft_lds dispatch is stonemask_kernel's switch.
template <int LO, int HI, class Fn>
int with_log2(int lg, Fn&& fn) {
  if constexpr (LO <= HI) return lg == LO ? fn(std::integral_constant<int, LO>{}) : with_log2<LO + 1, HI>(lg, fn);
  return PE_E_UNSUPPORTED;
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 conj2(float2 a) { return make_float2(a.x, -a.y); }
// multiply by -i
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }

// An LDS region that only one wave touches needs no s_barrier: a wave's DS instructions execute in program order,
// so a compiler fence that keeps LDS writes ahead of the dependent LDS reads is enough (the waves of a workgroup then
// drift freely instead of marching in lockstep).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// In-place C-point complex FFT (C = 2^LOG2C) of an LDS buffer that THREADS threads own: radix-4 Stockham passes and
// one radix-2 pass when LOG2C is odd (natural order in and out).  `tw`: the C-th roots of unity with the forward sign,
// conjugated here for INV; `tid` in [0, THREADS).  Every thread reads all inputs of its butterflies j = tid + THREADS b
// before the owners meet, then it writes: one buffer suffices.  THREADS == 64 is one wave on a region private to it,
// which meets at wave_lds_sync(); any other count is the whole workgroup, which meets at __syncthreads().
template <int LOG2C, bool INV, int THREADS>
__device__ __forceinline__ void fft_lds(float2* buf, const float2* tw, int tid) {
  constexpr int C = 1 << LOG2C, P4 = LOG2C / 2;
  constexpr int NB4 = (C / 4 + THREADS - 1) / THREADS;
  auto sync = [] {
    if constexpr (THREADS == 64) wave_lds_sync(); else __syncthreads();
  };
#pragma unroll
  for (int p = 0; p < P4; ++p) {
    const int ns = 1 << (2 * p), shift = LOG2C - 2 - 2 * p;        // twiddle index r k C / (4 ns)
    float2 v[NB4][4];
#pragma unroll
    for (int b = 0; b < NB4; ++b) {
      const int j = tid + THREADS * b;
      if (j < C / 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[b][r] = buf[j + (C / 4) * r];
      }
    }
    sync();
#pragma unroll
    for (int b = 0; b < NB4; ++b) {
      const int j = tid + THREADS * b;
      if (j < C / 4) {
        const int k = j & (ns - 1);
#pragma unroll
        for (int r = 1; r < 4; ++r) {
          const float2 w = tw[(r * k) << shift];
          v[b][r] = cmul(v[b][r], INV ? conj2(w) : w);
        }
        const float2 t0 = cadd(v[b][0], v[b][2]), t1 = csub(v[b][0], v[b][2]), t2 = cadd(v[b][1], v[b][3]);
        const float2 d = csub(v[b][1], v[b][3]);
        const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);      // * (+i) / * (-i)
        const int o = ((j >> (2 * p)) << (2 * p + 2)) + k;
        buf[o] = cadd(t0, t2);
        buf[o + ns] = cadd(t1, t3);
        buf[o + 2 * ns] = csub(t0, t2);
        buf[o + 3 * ns] = csub(t1, t3);
      }
    }
    sync();
  }
  if (LOG2C & 1) {                                                  // last pass, ns = C / 2: out index = in index
    constexpr int NB2 = (C / 2 + THREADS - 1) / THREADS;
    float2 a[NB2], b2[NB2];
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
      const int j = tid + THREADS * b;
      if (j < C / 2) {
        const float2 w = tw[j];
        a[b] = buf[j];
        b2[b] = cmul(buf[j + C / 2], INV ? conj2(w) : w);
      }
    }
    sync();
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
      const int j = tid + THREADS * b;
      if (j < C / 2) {
        buf[j] = cadd(a[b], b2[b]);
        buf[j + C / 2] = csub(a[b], b2[b]);
      }
    }
    sync();
  }
}

// A real signal of 2C samples packed as C complex points z[n] = x[2n] + i x[2n + 1] and transformed: with zk = Z[k]
// and zc = conj(Z[(C - k) mod C]), e = (zk + zc) / 2 and o = (zk - zc) / 2i are the transforms of the even and the
// odd samples, and bin k of the real transform is e + w o with w = exp(-2 pi i k / 2C).
__device__ __forceinline__ void real_fft_split(float2 zk, float2 zc, float2& e, float2& o) {
  e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
  const float2 dd = csub(zk, zc);
  o = make_float2(0.5f * dd.y, -0.5f * dd.x);
}

// Bin k < C of the real transform from the packed one in `z`, in halves: e and o as real_fft_split gives them, and
// the return value t = w o with w = tr[k] = exp(-2 pi i k / 2C).  X[k] = e + t and conj(X[C - k]) = e - t; at k = 0,
// X[0] = e.x + o.x and X[C] = e.x - o.x, both real (or X[C] = e + t from k = 0 with w = tr[C]).  How the halves are put
// together is the caller's.
__device__ __forceinline__ float2 real_fft_bin(const float2* z, float2 w, int C, int k, float2& e, float2& o) {
  real_fft_split(z[k], conj2(z[(C - k) & (C - 1)]), e, o);
  return cmul(w, o);
}

// The way back: the packed transform's bin k, E + i O, from y1 = Y[k] and y2 = conj(Y[C - k]) of a real signal's
// spectrum Y and w = tr[k]; the inverse C-point transform of these is the signal (times C).
__device__ __forceinline__ float2 real_fft_pack(float2 y1, float2 y2, float2 w) {
  const float2 ye = make_float2(0.5f * (y1.x + y2.x), 0.5f * (y1.y + y2.y));
  const float2 yo = cmul(make_float2(0.5f * (y1.x - y2.x), 0.5f * (y1.y - y2.y)), conj2(w));
  return make_float2(ye.x - yo.y, ye.y + yo.x);
}

// Reductions over a workgroup of 256 threads (four waves) in a fixed order; every thread gets the result.  s_red: 4
// floats that nothing else uses; the barrier ahead of the store lets a loop call these again without one of its own.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float block_sum(float v, float* s_red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__device__ __forceinline__ float block_max(float v, float* s_red, int tid) {
  v = wave_max(v);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// Standard normal for sample i of a row (world_synth.hip's pulse noise, noise.hip): Philox4x32-10 keyed by (seed, i),
// words 0 and 1, Box-Muller in float32.  A row's draws depend on its seed and the sample index alone.
__device__ __forceinline__ float world_randn(uint64_t seed, uint64_t i) {
  uint32_t w[4];
  philox4(seed, i, w);
  const float u1 = ((float)(w[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);       // (0, 1)
  const float u2 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);                // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// Largest row whose prefix offset meta[row][field] <= g, in a plan of `fields` int64 per row (rows with no work share
// the next row's offset).
__device__ __forceinline__ int find_row(const long* __restrict__ meta, int n_rows, int fields, int field, long g) {
  int lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (meta[(long)mid * fields + field] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace pe
