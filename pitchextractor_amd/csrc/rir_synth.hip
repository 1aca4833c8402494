// Room impulse responses of shoebox rooms by the image-source method (Allen & Berkley 1979) with a windowed-sinc
// fractional delay, and their decay time by Schroeder backward integration: the impulse responses that the reference's
// Utils/room_and_microphone_stress.ipynb reads from nine files nobody ships.  Pinned by the float64 restatement in
// tests/rir_ref.py.
//
// One row is one response.  Its parameters are doubles, P_K per row: room L, source s, microphone r, the six wall
// coefficients beta[a][0] (wall at 0) and beta[a][1] (wall at L_a), fs, c, the length N and max_order (-1: none).
//   image (n, p), n in Z^3, p in {0, 1}^3:  R_a = (1 - 2 p_a) s_a + 2 n_a L_a - r_a,  d = |R|,  tau = d fs / c,
//   A = prod_a beta[a][0]^|n_a - p_a| beta[a][1]^|n_a| / (4 pi d), 0^0 = 1; nothing from an image with A == 0, with
//   tau >= N + 41 or with sum_a |n_a - p_a| + |n_a| > max_order;
//   tap k, 0 <= k < N, x = k - tau, |x| < 41:  v = A sinc(x) (1 + cos(pi x / 41)) / 2;
//   h[k] = float32(2^-44 sum rint(2^44 v)), the sum over 64-bit integers.
// Integer addition is associative, so a sample does not depend on the order the images arrive in, on the work split
// or on the row's place in a batch, and the kernel needs no float atomics.
//
// pe_rir_plan (host only) checks the rooms and lays out the rows and the tile table: a tile is kTile consecutive
// samples of one row, the table is sorted by an estimate of the tile's images, (k1 c / fs)^2 (c / fs) / V, heaviest
// first, since a late tile holds ~t^2 more images than an early one.  pe_rir_synth is one launch of one workgroup per
// tile whatever the rows; no workgroup talks to another.  The workgroup owns the samples [k0, k1) of its row as long
// long accumulators in LDS.  Only images with tau in (k0 - 41, k1 + 40) can reach it: a shell of radii dlo .. dhi (one
// sample of slack each side).  With the lattice index i = 2 n - p per axis (p = i & 1, n = (i + p) / 2) the threads
// walk the columns (ix, iy) of the box that holds the shell's disc, skip those whose horizontal distance is beyond
// dhi, and for p_z = 0, 1 solve the two n_z intervals |R_z| in [zlo, zhi] (made disjoint, one extra index each side).
// Every candidate is then tested exactly; its taps with k in the tile are added by LDS integer atomics.  Ownership is
// by k, so every (image, tap) pair is added exactly once, also when an image straddles a tile edge.
// A tap is evaluated in double from f = tau - floor(tau): with x = j - f, sin(pi x) = -(-1)^j sin(pi f), one sinpi per
// image, and cos(pi x / 41) = C_j cos(pi f / 41) + S_j sin(pi f / 41) from the table C_j, S_j = cos, sin(pi j / 41)
// that the workgroup makes in LDS.  f == 0 is one tap, v = A, and no division by zero.
//
// pe_rir_decay: one workgroup per row.  E[k] = sum_{m >= k} h[m]^2 in double (a thread sums its run of consecutive
// samples, the runs are suffix-summed in thread order), db[k] = 10 log10(E[k] / E[0]); k_lo, k_hi = the first k with
// db < lo_db, hi_db (N when there is none); the least-squares line of db over k / fs on [k_lo, k_hi).
#include <math.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "pieces.h"

using namespace pe;

namespace {

// a decay workgroup is the kThreads of pieces.h, whose block_sum_d it takes
constexpr int kSynthThreads = 1024;              // of a tile's workgroup: four waves per SIMD under the long double chains
constexpr int kTile = 256;                       // samples of one tile: 2 KiB of LDS accumulators
constexpr int kHalf = 41;                        // half-width of the windowed sinc, in samples
constexpr double kFix = 17592186044416.0;        // 2^44, the fixed-point grid of the image sum
constexpr double kHeadroom = 262144.0;           // 2^18: the bound on sum |A| that pe_rir_plan accepts (2^63 / 2^44 = 2^19)
constexpr double kMaxIndex = 1073741824.0;       // 2^30: lattice indices stay in int
constexpr long kMaxLength = 1L << 24;            // samples of a row
constexpr long kMaxTiles = 1L << 20;
constexpr double kPi = 3.14159265358979323846;

enum { P_L, P_S = 3, P_R = 6, P_BETA = 9, P_FS = 15, P_C, P_N, P_ORDER, P_K };      // beta: [a][0], [a][1] at 9 + 2 a
enum { M_OFF, M_N, M_TILES, M_TOFF, M_K };
static_assert(M_OFF == kRowOffset && M_N == kRowLength, "the plan opens with the shared row header");
enum { T_ROW, T_K0, T_K };
enum { D_T60, D_SLOPE, D_ICPT, D_KLO, D_KHI, D_LAST, D_K };
enum { TOT_SAMPLES, TOT_TILES };

// PE_OK, PE_E_ARG or PE_E_UNSUPPORTED for one room
int check_room(const double* p) {
  for (int j = 0; j < P_K; ++j)
    if (!isfinite(p[j])) return PE_E_ARG;
  double gap2 = 0.0, diag2 = 0.0, vol = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double L = p[P_L + a], s = p[P_S + a], r = p[P_R + a];
    if (!(L > 0.0) || !(s > 0.0 && s < L) || !(r > 0.0 && r < L)) return PE_E_ARG;
    gap2 += (s - r) * (s - r); diag2 += L * L; vol *= L;
  }
  if (!(gap2 >= 1e-4)) return PE_E_ARG;                                // source and microphone at least 1 cm apart
  for (int j = 0; j < 6; ++j)
    if (!(p[P_BETA + j] >= 0.0 && p[P_BETA + j] <= 1.0)) return PE_E_ARG;
  if (!(p[P_FS] > 0.0) || !(p[P_C] > 0.0)) return PE_E_ARG;
  if (!(p[P_N] >= 1.0) || p[P_N] != floor(p[P_N])) return PE_E_ARG;
  if (!(p[P_ORDER] >= -1.0) || p[P_ORDER] != floor(p[P_ORDER])) return PE_E_ARG;
  if (p[P_N] > (double)kMaxLength || p[P_ORDER] > kMaxIndex) return PE_E_UNSUPPORTED;
  const double D = sqrt(diag2), dmax = (p[P_N] + kHalf + 1) * p[P_C] / p[P_FS];
  for (int a = 0; a < 3; ++a)
    if (!((dmax + D) / p[P_L + a] + 8.0 < kMaxIndex)) return PE_E_UNSUPPORTED;
  // every image lies in its own mirrored copy of the room (diagonal D, volume V) and is at least as far as the direct
  // path, >= 1 cm, so A < 8.  Images nearer than 2 D: their copies lie inside the ball of radius 3 D, at most
  // 36 pi D^3 / V of them.  Farther ones: 1 / (4 pi d) <= 2 / (4 pi rho) at every point of the copy (rho <= d + D <=
  // 2 d), so their sum is below the integral of 2 / (4 pi rho) dV / V = (dmax + D)^2 / V.
  const double bound = 8.0 * 36.0 * kPi * D * D * D / vol + (dmax + D) * (dmax + D) / vol;
  if (!(bound < kHeadroom)) return PE_E_UNSUPPORTED;
  return PE_OK;
}

long tiles_of(long n) { return (n + kTile - 1) / kTile; }

// rows and tile table of host params and offsets; tiles may be null (the totals only)
int lay_out(int n_rows, const double* params, const long* y_off, long* meta, long* tiles, long tile_capacity,
            long* totals2) {
  long s = 0, t = 0;
  for (int r = 0; r < n_rows; ++r) {
    const int st = check_room(params + (long)r * P_K);
    if (st != PE_OK) return st;
    if (y_off[r] < 0) return PE_E_ARG;
    long* m = meta + (long)r * M_K;
    m[M_OFF] = y_off[r]; m[M_N] = (long)params[(long)r * P_K + P_N]; m[M_TILES] = tiles_of(m[M_N]); m[M_TOFF] = t;
    s += m[M_N]; t += m[M_TILES];
    if (t > kMaxTiles) return PE_E_UNSUPPORTED;
  }
  totals2[TOT_SAMPLES] = s; totals2[TOT_TILES] = t;
  if (!tiles) return PE_OK;
  if (tile_capacity < t) return PE_E_ARG;
  struct Item { double w; long row, k0; };
  std::vector<Item> items;
  items.reserve((size_t)t);
  for (int r = 0; r < n_rows; ++r) {
    const double* p = params + (long)r * P_K;
    const double step = p[P_C] / p[P_FS], vol = p[P_L] * p[P_L + 1] * p[P_L + 2];
    const long n = meta[(long)r * M_K + M_N];
    for (long k0 = 0; k0 < n; k0 += kTile) {
      const double k1 = (double)(k0 + kTile < n ? k0 + kTile : n);
      items.push_back({k1 * step * k1 * step * step / vol, r, k0});
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.w > b.w; });
  for (long i = 0; i < t; ++i) { tiles[i * T_K + T_ROW] = items[(size_t)i].row; tiles[i * T_K + T_K0] = items[(size_t)i].k0; }
  return PE_OK;
}

// a^e for an integer e >= 0 as pow gives it (0^0 = 1)
__device__ __forceinline__ double ipow(double a, long e) { return pow(a, (double)e); }
__device__ __forceinline__ long labs_d(long v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(kSynthThreads) void rir_synth_kernel(const long* __restrict__ meta,
                                                             const double* __restrict__ params,
                                                             const long* __restrict__ tiles, float* __restrict__ y) {
  __shared__ unsigned long long s_acc[kTile];
  __shared__ double s_cos[kHalf + 1], s_sin[kHalf + 1];
  const int tid = threadIdx.x;
  const long row = tiles[(long)blockIdx.x * T_K + T_ROW], k0 = tiles[(long)blockIdx.x * T_K + T_K0];
  const double* p = params + row * P_K;
  const long* m = meta + row * M_K;
  const long N = m[M_N], k1 = k0 + kTile < N ? k0 + kTile : N;
  for (int i = tid; i < kTile; i += kSynthThreads) s_acc[i] = 0ull;
  if (tid <= kHalf) sincospi((double)tid / (double)kHalf, &s_sin[tid], &s_cos[tid]);
  __syncthreads();

  const double Lx = p[P_L], Ly = p[P_L + 1], Lz = p[P_L + 2];
  const double sx = p[P_S], sy = p[P_S + 1], sz = p[P_S + 2], rx = p[P_R], ry = p[P_R + 1], rz = p[P_R + 2];
  const double fs = p[P_FS], c = p[P_C];
  const long max_order = (long)p[P_ORDER];
  const bool any_order = max_order < 0;
  const double step = c / fs;
  const double dlo = k0 - kHalf - 1 > 0 ? (double)(k0 - kHalf - 1) * step : 0.0, dhi = (double)(k1 + kHalf) * step;
  const double dlo2 = dlo * dlo, dhi2 = dhi * dhi;
  const double tau_lo = (double)(k0 - kHalf), tau_hi = (double)(k1 - 1 + kHalf);   // taps reach the tile for tau strictly between
  const long ix0 = (long)floor((rx - dhi) / Lx) - 2, ix1 = (long)ceil((rx + dhi) / Lx) + 2;
  const long iy0 = (long)floor((ry - dhi) / Ly) - 2, iy1 = (long)ceil((ry + dhi) / Ly) + 2;
  const long nx = ix1 - ix0 + 1, ncols = nx * (iy1 - iy0 + 1);

  for (long col = tid; col < ncols; col += kSynthThreads) {
    const long cy = col / nx, ix = ix0 + (col - cy * nx), iy = iy0 + cy;
    const long px = ix & 1, py = iy & 1, qx = (ix + px) >> 1, qy = (iy + py) >> 1;       // q: the lattice n
    const double Rx = (double)(1 - 2 * px) * sx + 2.0 * (double)qx * Lx - rx;
    const double Ry = (double)(1 - 2 * py) * sy + 2.0 * (double)qy * Ly - ry;
    const double h2 = Rx * Rx + Ry * Ry;
    if (h2 > dhi2) continue;
    const long oxy = labs_d(qx - px) + labs_d(qx) + labs_d(qy - py) + labs_d(qy);
    if (!any_order && oxy > max_order) continue;
    const double gxy = ipow(p[P_BETA], labs_d(qx - px)) * ipow(p[P_BETA + 1], labs_d(qx)) *
                       ipow(p[P_BETA + 2], labs_d(qy - py)) * ipow(p[P_BETA + 3], labs_d(qy));
    if (gxy == 0.0) continue;
    const double zhi = sqrt(dhi2 - h2), zlo = dlo2 > h2 ? sqrt(dlo2 - h2) : 0.0;
    for (long pz = 0; pz < 2; ++pz) {
      const double z0 = (double)(1 - 2 * pz) * sz - rz;
      // R_z = z0 + 2 n L_z in [-zhi, -zlo] and in [zlo, zhi]: two disjoint runs of n, one extra index each side
      long a0 = (long)floor((-zhi - z0) / (2.0 * Lz)) - 1, a1 = (long)ceil((-zlo - z0) / (2.0 * Lz)) + 1;
      long b0 = (long)floor((zlo - z0) / (2.0 * Lz)) - 1, b1 = (long)ceil((zhi - z0) / (2.0 * Lz)) + 1;
      if (b0 <= a1) b0 = a1 + 1;
      for (int side = 0; side < 2; ++side) {
        const long q0 = side ? b0 : a0, q1 = side ? b1 : a1;
        for (long qz = q0; qz <= q1; ++qz) {
          const double Rz = z0 + 2.0 * (double)qz * Lz;
          const double d = sqrt(h2 + Rz * Rz), tau = d * fs / c;
          if (!(tau > tau_lo && tau < tau_hi) || tau >= (double)(N + kHalf)) continue;
          const long ez0 = labs_d(qz - pz), ez1 = labs_d(qz);
          if (!any_order && oxy + ez0 + ez1 > max_order) continue;
          const double A = gxy * ipow(p[P_BETA + 4], ez0) * ipow(p[P_BETA + 5], ez1) / (4.0 * kPi * d);
          if (!(A * kFix >= 0.5)) continue;                              // every tap of it rounds to 0 (|v| <= A)
          const double fl = floor(tau), f = tau - fl;
          const long mk = (long)fl;
          if (f == 0.0) {                                                // an integer delay: the one tap x = 0
            if (mk >= k0 && mk < k1) atomicAdd(&s_acc[mk - k0], (unsigned long long)llrint(A * kFix));
            continue;
          }
          double sf, cf;
          sincospi(f / (double)kHalf, &sf, &cf);
          const double amp = A * sinpi(f) / kPi * 0.5;
          long j0 = -(kHalf - 1), j1 = kHalf;                            // |j - f| < 41 for 0 < f < 1
          if (mk + j0 < k0) j0 = k0 - mk;
          if (mk + j1 > k1 - 1) j1 = k1 - 1 - mk;
          for (long j = j0; j <= j1; ++j) {
            const int ja = (int)(j < 0 ? -j : j);
            const double sj = j < 0 ? -s_sin[ja] : s_sin[ja];
            const double hann2 = 1.0 + (s_cos[ja] * cf + sj * sf);       // 1 + cos(pi (j - f) / 41)
            const double sinc_pi = ((j & 1) ? -amp : amp) / (f - (double)j);
            atomicAdd(&s_acc[mk + j - k0], (unsigned long long)llrint(sinc_pi * hann2 * kFix));
          }
        }
      }
    }
  }
  __syncthreads();
  float* out = y + m[M_OFF];
  for (long i = tid; k0 + i < k1; i += kSynthThreads)
    out[k0 + i] = (float)((double)(long long)s_acc[i] * (1.0 / kFix));
}

// Suffix sums of one double per thread in thread order: s_run[t] = sum of the values of threads >= t (s_run[kThreads]
// = 0).  Thread 0 adds them one by one.
__device__ __forceinline__ void suffix_runs(double v, double* s_run, int tid) {
#pragma clang fp contract(off)
  s_run[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    s_run[kThreads] = 0.0;
    for (int t = kThreads - 1; t >= 0; --t) { acc += s_run[t]; s_run[t] = acc; }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void rir_decay_kernel(const float* __restrict__ h,
                                                             const long* __restrict__ meta, int meta_fields, double fs,
                                                             double lo_db, double hi_db, double* __restrict__ out,
                                                             float* __restrict__ curve) {
#pragma clang fp contract(off)
  __shared__ double s_run[kThreads + 1];
  __shared__ double s_sum[kThreads];
  __shared__ long s_first[2][kThreads];
  const int tid = threadIdx.x, row = blockIdx.x;
  const long* m = meta + (long)row * meta_fields;
  const long N = m[kRowLength];
  const float* x = h + m[kRowOffset];
  double* o = out + (long)row * D_K;
  if (N < 1) {
    if (tid == 0) { o[D_T60] = o[D_SLOPE] = o[D_ICPT] = o[D_LAST] = nan(""); o[D_KLO] = o[D_KHI] = 0.0; }
    return;
  }
  const long run = (N + kThreads - 1) / kThreads;
  const long b = (long)tid * run < N ? (long)tid * run : N, e = b + run < N ? b + run : N;
  double own = 0.0;
  for (long k = e - 1; k >= b; --k) { const double v = (double)x[k]; own += v * v; }
  suffix_runs(own, s_run, tid);
  const double E0 = s_run[0];
  // the first index of the thread's run below each threshold (db does not rise with k)
  long first_lo = N, first_hi = N;
  double acc = s_run[tid + 1], last_db = 0.0;
  for (long k = e - 1; k >= b; --k) {
    const double v = (double)x[k];
    acc += v * v;
    const double db = 10.0 * log10(acc / E0);
    if (k == N - 1) last_db = db;
    if (db < lo_db) first_lo = k;
    if (db < hi_db) first_hi = k;
    if (curve) curve[m[kRowOffset] + k] = (float)db;
  }
  s_first[0][tid] = first_lo; s_first[1][tid] = first_hi;
  if (e == N && b < N) s_sum[0] = last_db;                               // the one thread that holds sample N - 1
  __syncthreads();
  long k_lo = N, k_hi = N;
  for (int t = 0; t < kThreads; ++t) {
    if (s_first[0][t] < k_lo) k_lo = s_first[0][t];
    if (s_first[1][t] < k_hi) k_hi = s_first[1][t];
  }
  const double db_last = s_sum[0];
  __syncthreads();
  // least squares of db over u = k - k_lo on [k_lo, k_hi)
  double su = 0.0, suu = 0.0, sd = 0.0, sud = 0.0;
  acc = s_run[tid + 1];
  for (long k = e - 1; k >= b; --k) {
    const double v = (double)x[k];
    acc += v * v;
    if (k >= k_lo && k < k_hi) {
      const double u = (double)(k - k_lo), db = 10.0 * log10(acc / E0);
      su += u; suu += u * u; sd += db; sud += u * db;
    }
  }
  su = block_sum_d(su, s_sum, tid); suu = block_sum_d(suu, s_sum, tid);
  sd = block_sum_d(sd, s_sum, tid); sud = block_sum_d(sud, s_sum, tid);
  if (tid != 0) return;
  o[D_KLO] = (double)k_lo; o[D_KHI] = (double)k_hi; o[D_LAST] = db_last;
  const double cnt = (double)(k_hi - k_lo);
  if (!(E0 > 0.0) || k_hi >= N || k_hi - k_lo < 2) { o[D_T60] = o[D_SLOPE] = o[D_ICPT] = nan(""); return; }
  const double per_sample = (cnt * sud - su * sd) / (cnt * suu - su * su);           // dB per sample
  const double slope = per_sample * fs;
  o[D_SLOPE] = slope;
  o[D_ICPT] = (sd - per_sample * su) / cnt - per_sample * (double)k_lo;
  o[D_T60] = -60.0 / slope;
}

}  // namespace

extern "C" int pe_rir_plan_fields(void) { return M_K; }

/* Host-only checks and layout; see include/pitchextractor_hip.h. */
extern "C" int pe_rir_plan(int n_rows, const double* params, const long* y_off, long* consts4, long* meta,
                           long* tiles, long tile_capacity, long* totals2) {
  if (!consts4 || !totals2 || n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  consts4[0] = kTile; consts4[1] = P_K; consts4[2] = T_K; consts4[3] = D_K;
  totals2[TOT_SAMPLES] = totals2[TOT_TILES] = 0;
  if (n_rows == 0) return PE_OK;
  if (!params || !y_off || !meta) return PE_E_ARG;
  return lay_out(n_rows, params, y_off, meta, tiles, tile_capacity, totals2);
}

extern "C" int pe_rir_synth(const long* meta, const long* host_meta, const double* params, const double* host_params,
                            const long* tiles, const long* host_tiles, int n_rows, float* y, long n_y, void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows) return PE_E_ARG;
  if (n_rows == 0) return PE_OK;
  if (!host_meta || !host_params || !host_tiles) return PE_E_ARG;
  // the host copies are the plan's: laid out again from the rooms and the offsets, they come out the same
  std::vector<long> off((size_t)n_rows), again((size_t)n_rows * M_K);
  long tot[2];
  for (int r = 0; r < n_rows; ++r) off[(size_t)r] = host_meta[(long)r * M_K + M_OFF];
  int st = lay_out(n_rows, host_params, off.data(), again.data(), nullptr, 0, tot);
  if (st != PE_OK) return st;
  if (memcmp(again.data(), host_meta, again.size() * sizeof(long)) != 0) return PE_E_ARG;
  std::vector<long> table((size_t)tot[TOT_TILES] * T_K);
  st = lay_out(n_rows, host_params, off.data(), again.data(), table.data(), tot[TOT_TILES], tot);
  if (st != PE_OK) return st;
  if (memcmp(table.data(), host_tiles, table.size() * sizeof(long)) != 0) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (off[(size_t)r] > n_y || again[(size_t)r * M_K + M_N] > n_y - off[(size_t)r]) return PE_E_ARG;
  if (!meta || !params || !tiles || !y) return PE_E_ARG;
  hipLaunchKernelGGL(rir_synth_kernel, dim3((unsigned)tot[TOT_TILES]), dim3(kSynthThreads), 0, pe_stream(stream),
                     meta, params, tiles, y);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_rir_decay(const float* h, long n_h, const long* meta, const long* host_meta, int meta_fields,
                            int n_rows, double fs, double lo_db, double hi_db, double* out6, float* curve,
                            void* stream) {
  if (n_rows < 0 || n_rows > kMaxRows || meta_fields < kRowHeader) return PE_E_ARG;
  if (!(fs > 0.0) || !isfinite(fs) || !isfinite(lo_db) || !isfinite(hi_db) || !(hi_db < lo_db) || !(lo_db <= 0.0))
    return PE_E_ARG;
  if (n_rows == 0) return PE_OK;
  if (!host_meta) return PE_E_ARG;
  for (int r = 0; r < n_rows; ++r) {
    const long off = host_meta[(long)r * meta_fields + kRowOffset], n = host_meta[(long)r * meta_fields + kRowLength];
    if (off < 0 || n < 0 || n > (1L << 31) - 8 || off > n_h || n > n_h - off) return PE_E_ARG;
  }
  if (!h || !meta || !out6) return PE_E_ARG;
  hipLaunchKernelGGL(rir_decay_kernel, dim3(n_rows), dim3(kThreads), 0, pe_stream(stream), h, meta, meta_fields, fs,
                     lo_db, hi_db, out6, curve);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
