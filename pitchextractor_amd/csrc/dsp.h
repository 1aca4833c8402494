// What the audio kernels (mel.hip, pitch_shift.hip, f0_track.hip, f0_dio.hip, world_synth.hip) share.  Host: the row
// bound and launch-grid clamp of the ragged entry points, the header every row plan opens with, and with_log2 (transform
// size -> kernel instance).  Device: float2 complex arithmetic, the wave-private LDS fence, the in-place radix-4 Stockham
// FFT in LDS, the split of a packed half-length transform into the real one's bins, and the row search of ragged plans.
#pragma once
#include <type_traits>
#include "common.h"

namespace pe {

constexpr int kMaxRows = 65535;           // rows of one ragged batch (a launch grid's y / x extent)
constexpr float kPiF = 3.14159265358979323846f;
// workgroups of a grid-stride launch over `items` work items
inline unsigned grid_of(long items) { return (unsigned)(items < (1L << 20) ? items : (1L << 20)); }

// Every row plan (n_rows x K int64, K the plan's own field count) opens with the row's offset in `x` and its length in
// samples.  A plan's enum static_asserts this; what reads only this header (pe_row_stats) serves any plan given its K.
enum { kRowOffset = 0, kRowLength = 1, kRowHeader = 2 };

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
