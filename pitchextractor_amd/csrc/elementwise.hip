// HBM-bound stages of the JDCNet stack on channels-last activations [rows = B*T][F][C]:
// train-mode BatchNorm2d statistics (model.py:25,37,54,150,159), the fused
// BN -> LeakyReLU(0.01) -> MaxPool2d((1, k)) blocks (model.py:36-41,148-153) forward and backward,
// the detector-branch max-pools (model.py:45-49), dropout (model.py:40,56) and the
// (B,256,T,2) -> (B,T,512) re-layout of model.py:93,112.  Everything moves float4 (4 channels).
#include <type_traits>
#include "forms.h"

namespace {
using namespace pe;

constexpr int kMaxPartials = 4096;

// ---------------------------------------------------------------- per-channel two-value reduction
// Each thread owns one channel quad and every G-th pixel; sums are kept in double so the biased
// variance E[x^2] - E[x]^2 loses nothing at 4M samples per channel.
template <class F>
__device__ __forceinline__ void column_reduce2(F&& f, long n_pix, int C, double* partial /*[grid][2][C]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* red = reinterpret_cast<double*>(smem_raw);            // [G][2][C]
  const int quads = C >> 2;
  const int G = 256 / quads;
  const int q = threadIdx.x % quads, g = threadIdx.x / quads;
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  if (g < G) {
    for (long p = (long)blockIdx.x * G + g; p < n_pix; p += (long)gridDim.x * G) {
      float4 a, b;
      f(p, q * 4, a, b);
      s1[0] += a.x; s1[1] += a.y; s1[2] += a.z; s1[3] += a.w;
      s2[0] += b.x; s2[1] += b.y; s2[2] += b.z; s2[3] += b.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[(g * 2 + 0) * C + q * 4 + i] = s1[i];
      red[(g * 2 + 1) * C + q * 4 + i] = s2[i];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    double s = 0;
    for (int gg = 0; gg < G; ++gg) s += red[gg * 2 * C + i];
    partial[(long)blockIdx.x * 2 * C + i] = s;
  }
}

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---------------------------------------------------------------- the per-quad rules every pass below shares
// BatchNorm (as the affine map scale * x + shift) and LeakyReLU of one channel quad
__device__ __forceinline__ float4 bn_lrelu4(const float4& v, const float4& sc, const float4& sh, float slope) {
  return make_float4(lrelu(fmaf(v.x, sc.x, sh.x), slope), lrelu(fmaf(v.y, sc.y, sh.y), slope),
                     lrelu(fmaf(v.z, sc.z, sh.z), slope), lrelu(fmaf(v.w, sc.w, sh.w), slope));
}

__device__ __forceinline__ float4 fmax4(const float4& a, const float4& b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// dx = gamma*invstd * (dz - mean(dz) - xhat * mean(dz*xhat)) of one quad: sc == gamma*invstd, k1 / k2 the two means
__device__ __forceinline__ float4 bn_dx4(const float4& dz, const float4& v, const float4& mu, const float4& is,
                                         const float4& sc, const float4& k1, const float4& k2) {
  return make_float4(sc.x * (dz.x - k1.x - (v.x - mu.x) * is.x * k2.x), sc.y * (dz.y - k1.y - (v.y - mu.y) * is.y * k2.y),
                     sc.z * (dz.z - k1.z - (v.z - mu.z) * is.z * k2.z), sc.w * (dz.w - k1.w - (v.w - mu.w) * is.w * k2.w));
}

// The first maximum of a window and its position, per channel of a quad: a strict > scanning upwards, so a tie stays
// with the lower position (where torch's max_pool2d backward routes the gradient), a NaN inside the window is skipped
// and one at the window's start sticks.  `force`: x is the window's first element and is taken whatever m holds.
// Every max-pool of this file, forward and backward, finds its maxima through this rule; the one place that spells
// it out again is the LDS fold of bn_act_pool_tap_fwd_kernel (see there).
__device__ __forceinline__ void first_max(float& m, int& at, float x, int pos, bool force = false) {
  if (force || x > m) { m = x; at = pos; }
}

// the running maxima of a channel quad and their positions
struct FirstMax4 {
  float4 v;
  int p0, p1, p2, p3;

  __device__ __forceinline__ static FirstMax4 at(const float4& x, int pos) { return FirstMax4{x, pos, pos, pos, pos}; }

  // one step: the quad x, found at position pos
  __device__ __forceinline__ void take(const float4& x, int pos, bool force = false) {
    first_max(v.x, p0, x.x, pos, force);
    first_max(v.y, p1, x.y, pos, force);
    first_max(v.z, p2, x.z, pos, force);
    first_max(v.w, p3, x.w, pos, force);
  }

  // rows 0 .. n-1 of a window that starts at xp, `stride` elements apart; four rows in flight
  template <class TA>
  __device__ __forceinline__ static FirstMax4 scan(const TA* xp, long stride, int n) {
    FirstMax4 m = at(ld4(xp), 0);
    int j = 1;
    for (; j + 4 <= n; j += 4) {
      float4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = ld4(xp + (long)(j + u) * stride);
#pragma unroll
      for (int u = 0; u < 4; ++u) m.take(x[u], j + u);
    }
    for (; j < n; ++j) m.take(ld4(xp + (long)j * stride), j);
    return m;
  }

  __device__ __forceinline__ uchar4 bytes() const {
    return make_uchar4((unsigned char)p0, (unsigned char)p1, (unsigned char)p2, (unsigned char)p3);
  }
};

// ---------------------------------------------------------------- BN statistics
template <class TA>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const TA* __restrict__ x, long n_pix, int C,
                                                               double* __restrict__ partial) {
  column_reduce2(
      [&](long p, int c, float4& a, float4& b) {
        a = ld4(x + p * C + c);
        b = make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w);
      },
      n_pix, C, partial);
}

// [nparts][2][C] -> [gridDim.x][2][C]: a thread owns one of the 2C columns, so every read is coalesced across the
// block; part p goes to block p % gridDim.x and is added in increasing p (fixed order: deterministic)
__global__ __launch_bounds__(256) void bn_partials_fold_kernel(const double* __restrict__ partial, int nparts, int C2,
                                                               double* __restrict__ out) {
  for (int col = threadIdx.x; col < C2; col += 256) {
    double s = 0.0;
    for (int p = blockIdx.x; p < nparts; p += gridDim.x) s += partial[(long)p * C2 + col];
    out[(long)blockIdx.x * C2 + col] = s;
  }
}

__global__ void bn_stats_finalize_kernel(const double* __restrict__ partial, int nparts, long n_pix, int C,
                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                         float momentum, float* __restrict__ running_mean,
                                         float* __restrict__ running_var, float* __restrict__ mean_out,
                                         float* __restrict__ invstd_out, float* __restrict__ scale,
                                         float* __restrict__ shift) {
  // one wave per channel (4 channels per 256-thread block)
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const double s1 = pe_wave_strided_sum(partial + c, 2L * C, nparts);
  const double s2 = pe_wave_strided_sum(partial + C + c, 2L * C, nparts);
  if ((threadIdx.x & 63) != 0) return;
  const double n = (double)n_pix;
  const double mean = s1 / n;
  double var = s2 / n - mean * mean;
  if (var < 0) var = 0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  mean_out[c] = (float)mean;
  invstd_out[c] = invstd;
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mean * sc;
  if (running_mean) {
    const double unbiased = n > 1 ? var * n / (n - 1.0) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

__global__ void bn_eval_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv, float eps, int C,
                                      float* __restrict__ scale, float* __restrict__ shift,
                                      float* __restrict__ mean, float* __restrict__ invstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = 1.0f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
  mean[c] = rm[c];                      // the statistics the layer normalised with: what its backward reads
  invstd_out[c] = invstd;
}

// ---------------------------------------------------------------- "h2" scale source from the producing pass
// A pass that writes a tensor a later fp32 product reads can leave the tensor's largest magnitude behind: every
// thread keeps max |v| of what it stores (v_max_f32 with |.| source modifiers), the workgroup folds it and one
// no-return atomicMax per workgroup merges the IEEE bit patterns (ordered like unsigned integers) into *amax, a
// word the caller zeroed.  Exact and order-independent; the separate pe_absmax pass over the tensor disappears.
__device__ __forceinline__ float amax4(float m, const float4& v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

__device__ __forceinline__ void amax_commit(float m, unsigned* __restrict__ amax) {
  if (amax == nullptr) return;                                   // (uniform across the grid)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  __shared__ float amax_red[4];
  if ((threadIdx.x & 63) == 0) amax_red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float w = fmaxf(fmaxf(amax_red[0], amax_red[1]), fmaxf(amax_red[2], amax_red[3]));
    atomicMax(amax, __float_as_uint(w));
  }
}

// ---------------------------------------------------------------- BN -> LReLU -> MaxPool(1,k) forward
// x: [rows][Fin][C]; y: pixel (row, fo) at y[(row*Fout + fo)*ldy + coff + c]
template <class TA>
__global__ __launch_bounds__(256) void bn_act_pool_fwd_kernel(const TA* __restrict__ x,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float slope,
                                                              TA* __restrict__ y, long n_out_pix, int Fin, int C,
                                                              int pool, long ldy, int coff,
                                                              unsigned* __restrict__ amax) {
  const int quads = C >> 2;
  const int Fout = Fin / pool;
  float am = 0.f;
  // thread = (channel quad q, pixel lane g): a thread's quad never changes, so its per-channel vectors are loaded once,
  // not per pixel (with bf16 tensors they were most of the bytes a thread requested); 256 / quads pixels per block and
  // trip (C = 192: 5 pixels, 16 idle threads)
  const int G = 256 / quads, q = threadIdx.x % quads, g = threadIdx.x / quads;
  const float4 sc = *reinterpret_cast<const float4*>(scale + q * 4), sh = *reinterpret_cast<const float4*>(shift + q * 4);
  for (long op = (long)blockIdx.x * G + g; g < G && op < n_out_pix; op += (long)gridDim.x * G) {
    const long row = op / Fout;
    const int fo = (int)(op % Fout);
    const TA* xp = x + ((row * Fin + (long)fo * pool) * C + q * 4);
    float4 m;
    for (int j = 0; j < pool; ++j) {
      const float4 a = bn_lrelu4(ld4(xp + (long)j * C), sc, sh, slope);
      m = j == 0 ? a : fmax4(m, a);
    }
    st4(y + op * ldy + coff + q * 4, m);
    am = amax4(am, m);
  }
  amax_commit(am, amax);
}

// The same pass with a detector tap folded in: the plain MaxPool(1, tap_pool) of the raw x it reads anyway, written at
// tap_y[tw*tap_ldy + tap_coff + c] (tw = row*Fo_tap + w), and the window position of each maximum at tap_arg[tw*C + c],
// exactly as maxpool_fwd_kernel leaves them (strict > scanning upwards: the first maximum wins, value = the x bits).
// Fin % tap_pool == 0 and tap_pool % POOL == 0, so tap window tw is the x pixels [tw*tap_pool, (tw+1)*tap_pool) and the
// BN windows [tw*nbw, (tw+1)*nbw): no division anywhere.  A tap window is cut into S segments of segw = nbw / S BN
// windows; pixel lane g of a trip owns segment g % S of tap window trip*TW + g / S (TW = G / S windows per trip; the
// host picks S so that TW*S fills the lanes).  Every lane scans its segment upwards, the (value, position) pairs meet
// in LDS and the lane of segment 0 folds them in segment order with the same strict >, which keeps the first-maximum
// rule (a later segment starts from -inf, so a NaN inside a window is skipped and one at position 0 sticks, as in the
// serial scan).  The LDS buffers alternate by trip: one barrier per trip.
template <int POOL, class TA>
__global__ __launch_bounds__(256) void bn_act_pool_tap_fwd_kernel(const TA* __restrict__ x,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, float slope,
                                                                  TA* __restrict__ y, long n_tap, int C, int nbw, int S,
                                                                  long ldy, int coff, unsigned* __restrict__ amax,
                                                                  TA* __restrict__ tap_y, long tap_ldy, int tap_coff,
                                                                  unsigned char* __restrict__ tap_arg) {
  __shared__ float4 tap_val[2][256];
  __shared__ uchar4 tap_pos[2][256];
  const int quads = C >> 2;
  const int G = 256 / quads, q = threadIdx.x % quads, g = threadIdx.x / quads;
  const int TW = G / S, segw = nbw / S;
  const int wl = g / S, seg = g - wl * S;
  const bool lane_on = g < TW * S;
  const float4 sc = *reinterpret_cast<const float4*>(scale + q * 4), sh = *reinterpret_cast<const float4*>(shift + q * 4);
  const long n_trips = (n_tap + TW - 1) / TW;
  float am = 0.f;
  int buf = 0;
  for (long trip = blockIdx.x; trip < n_trips; trip += gridDim.x, buf ^= 1) {
    const long tw = trip * TW + wl;
    const bool on = lane_on && tw < n_tap;
    const float ninf = -__builtin_inff();
    FirstMax4 tm = FirstMax4::at(make_float4(ninf, ninf, ninf, ninf), seg * segw * POOL);
    if (on) {
      const long op0 = tw * nbw + (long)seg * segw;
      const TA* xp = x + (op0 * POOL * C + q * 4);
      TA* yp = y + (op0 * ldy + coff + q * 4);
      int pos = seg * segw * POOL;
      bool first = seg == 0;                                       // the scan of a window starts AT its first element
      for (int i = 0; i < segw; ++i, xp += (long)POOL * C, yp += ldy) {
        float4 v[POOL];
#pragma unroll
        for (int j = 0; j < POOL; ++j) v[j] = ld4(xp + (long)j * C);
        float4 m;
#pragma unroll
        for (int j = 0; j < POOL; ++j, ++pos) {
          const float4 a = bn_lrelu4(v[j], sc, sh, slope);
          m = j == 0 ? a : fmax4(m, a);
          tm.take(v[j], pos, first);
          first = false;
        }
        st4(yp, m);
        am = amax4(am, m);
      }
      if (S > 1) {
        tap_val[buf][threadIdx.x] = tm.v;
        tap_pos[buf][threadIdx.x] = tm.bytes();
      }
    }
    if (S > 1) __syncthreads();
    if (on && seg == 0) {
      for (int k = 1; k < S; ++k) {                                // segments in window order: a tie stays with the lower one
        const float4 o = tap_val[buf][threadIdx.x + k * quads];
        const uchar4 p = tap_pos[buf][threadIdx.x + k * quads];
        // first_max written out: the positions are converted inside the branches, so the compiler reads them from LDS
        // byte by byte and only where taken; handed to first_max as ints they become one word read per segment and
        // another kernel (71 -> 56..60 VGPRs at POOL = 1, other occupancies), which has not been timed
        if (o.x > tm.v.x) { tm.v.x = o.x; tm.p0 = p.x; }
        if (o.y > tm.v.y) { tm.v.y = o.y; tm.p1 = p.y; }
        if (o.z > tm.v.z) { tm.v.z = o.z; tm.p2 = p.z; }
        if (o.w > tm.v.w) { tm.v.w = o.w; tm.p3 = p.w; }
      }
      st4(tap_y + tw * tap_ldy + tap_coff + q * 4, tm.v);
      if (tap_arg != nullptr) *reinterpret_cast<uchar4*>(tap_arg + tw * C + q * 4) = tm.bytes();
    }
  }
  amax_commit(am, amax);
}

// ---------------------------------------------------------------- BN -> LReLU -> MaxPool(1,k) backward, k in {1, 2, 4}
template <class TA>
struct BnBwdArgsT {
  const TA* x;          // [rows][Fin][C]
  const TA* dy;         // pixel (row, fo) at dy[(row*Fout + fo)*lddy + coff + c]
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  float slope;
  long n_in_pix;        // rows * Fin
  int Fin, C;
  long lddy;
  int coff;
};

__global__ void bn_bwd_finalize_kernel(const double* __restrict__ partial, int nparts, long n_pix, int C,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta,
                                       float* __restrict__ c1, float* __restrict__ c2) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const double s1 = pe_wave_strided_sum(partial + c, 2L * C, nparts);
  const double s2 = pe_wave_strided_sum(partial + C + c, 2L * C, nparts);
  if ((threadIdx.x & 63) != 0) return;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  if (c1 == nullptr) return;            // running statistics: the input gradient has no mean / projection term
  c1[c] = (float)(s1 / (double)n_pix);
  c2[c] = (float)(s2 / (double)n_pix);
}

// The means of bn_dx4.  With running statistics (eval mode) the layer is the affine map z = scale * x + shift and
// dx = scale * dz: the apply pass runs with c1 == c2 == nullptr, which stands for two zero vectors
// (dz - 0 - xhat * 0 == dz exactly).
__device__ __forceinline__ float4 bn_term(const float* __restrict__ k, int c) {
  return k != nullptr ? *reinterpret_cast<const float4*>(k + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The two backward passes (per-channel sums, then dx) in window form: one thread owns a whole pool window of a
// channel quad, so x is read exactly once per pass (float4, coalesced along C), the arg-max is found once
// and only one 64-bit division is paid per window.  Item w of a row is window w for w < Fout, plus one
// trailing item for the floor-mode remainder pixels (dz = 0, but they count in the means and get a dx).
template <int POOL>
struct BnWindow {
  float4 v[POOL], dz[POOL];
  long p0;       // first input pixel of the item
  int n;         // pixels in it
};

template <int POOL, class TA>
__device__ __forceinline__ void bn_window(const BnBwdArgsT<TA>& a, long item, int nwin, int c, BnWindow<POOL>& w,
                                          const float4& sc, const float4& sh) {
  const int Fout = a.Fin / POOL;
  const long row = item / nwin;
  const int wi = (int)(item - row * nwin);
  const bool real = wi < Fout;
  w.n = real ? POOL : a.Fin - Fout * POOL;
  w.p0 = row * a.Fin + (long)wi * POOL;
  const TA* xp = a.x + w.p0 * a.C + c;
#pragma unroll
  for (int j = 0; j < POOL; ++j) {
    w.v[j] = j < w.n ? ld4(xp + (long)j * a.C) : make_float4(0.f, 0.f, 0.f, 0.f);
    w.dz[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (!real) return;
  const float4 dyv = ld4(a.dy + (row * Fout + wi) * a.lddy + a.coff + c);
  // bn_lrelu4 of the window's quads, channel by channel: computed as whole quads up front the six pooled instances
  // come out with other registers (apply_win<4>: 80 -> 88..90 VGPRs, occupancy 6 -> 5), so the scalar form stays
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float dys[4] = {dyv.x, dyv.y, dyv.z, dyv.w};
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    float best = lrelu(fmaf(reinterpret_cast<const float*>(&w.v[0])[ch], scv[ch], shv[ch]), a.slope);
    int arg = 0;
#pragma unroll
    for (int j = 1; j < POOL; ++j)
      first_max(best, arg, lrelu(fmaf(reinterpret_cast<const float*>(&w.v[j])[ch], scv[ch], shv[ch]), a.slope), j);
    const float g = best > 0.f ? dys[ch] : dys[ch] * a.slope;  // sign(lrelu(z)) == sign(z)
#pragma unroll
    for (int j = 0; j < POOL; ++j) reinterpret_cast<float*>(&w.dz[j])[ch] = j == arg ? g : 0.f;
  }
}

template <int POOL, class TA>
__global__ __launch_bounds__(256) void bn_bwd_partial_win_kernel(const BnBwdArgsT<TA> a, long n_items, int nwin,
                                                                 double* __restrict__ partial) {
  const int c0 = (threadIdx.x % (a.C >> 2)) * 4;               // column_reduce2 hands this thread no other quad
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + c0), is = *reinterpret_cast<const float4*>(a.invstd + c0);
  const float4 sc = *reinterpret_cast<const float4*>(a.scale + c0), sh = *reinterpret_cast<const float4*>(a.shift + c0);
  column_reduce2(
      [&](long item, int c, float4& s, float4& t) {
        BnWindow<POOL> w;
        bn_window<POOL, TA>(a, item, nwin, c, w, sc, sh);
        s = make_float4(0.f, 0.f, 0.f, 0.f);
        t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < POOL; ++j) {                      // one dz per channel is non-zero: plain fp32 sums are exact
          s.x += w.dz[j].x; s.y += w.dz[j].y; s.z += w.dz[j].z; s.w += w.dz[j].w;
          t.x += w.dz[j].x * ((w.v[j].x - mu.x) * is.x); t.y += w.dz[j].y * ((w.v[j].y - mu.y) * is.y);
          t.z += w.dz[j].z * ((w.v[j].z - mu.z) * is.z); t.w += w.dz[j].w * ((w.v[j].w - mu.w) * is.w);
        }
      },
      n_items, a.C, partial);
}

// The gradient of a detector tap (the plain MaxPool(1, tap_pool) of x, see bn_act_pool_tap_fwd_kernel) for the apply pass
// to add to the dx it writes: dy of tap window tw at dy[tw*lddy + coff + c], the position of its maximum at arg[tw*C + c].
template <class TA>
struct BnTapGrad {
  const TA* dy;
  const unsigned char* arg;
  long lddy;
  int coff;
  unsigned nbw;         // BN windows per tap window (tap_pool / POOL)
};

// stored element + tap gradient as the separate pass adds them: the element rounded to its storage type first, and an
// add of its own (fused into the multiply that produced dx it would round once instead of twice)
__device__ __forceinline__ float round_act(const float*, float v) { return v; }
__device__ __forceinline__ float round_act(const act16_t*, float v) {          // what st4 stores, widened again
  return __uint_as_float(pack_bf16_rne(v, 0.f) << 16);
}
__device__ __forceinline__ float add_unfused(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The apply pass: dx of every window, and with a tap (Tap = BnTapGrad<TA>; NoTap: none) the tap's gradient added to the
// element it belongs to.  Fin % tap_pool == 0 and n_items < 2^31 (the host checks both), so BN window `item` of the
// whole tensor lies in tap window item / nbw, at positions pos0 .. pos0 + POOL - 1 of it.
struct NoTap {};

template <int POOL, class TA, class Tap>
__device__ __forceinline__ void bn_bwd_apply_win(const BnBwdArgsT<TA>& a, long n_items, int nwin,
                                                 const float* __restrict__ c1, const float* __restrict__ c2,
                                                 TA* __restrict__ dx, unsigned* __restrict__ amax, const Tap& t) {
  constexpr bool TAP = !std::is_same<Tap, NoTap>::value;
  const int quads = a.C >> 2;
  float am = 0.f;
  const int G = 256 / quads, c = (threadIdx.x % quads) * 4, g = threadIdx.x / quads;     // see bn_act_pool_fwd_kernel
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + c), is = *reinterpret_cast<const float4*>(a.invstd + c);
  const float4 sc = *reinterpret_cast<const float4*>(a.scale + c), sh = *reinterpret_cast<const float4*>(a.shift + c);
  const float4 k1 = bn_term(c1, c), k2 = bn_term(c2, c);
  for (long item = (long)blockIdx.x * G + g; g < G && item < n_items; item += (long)gridDim.x * G) {
    BnWindow<POOL> w;
    bn_window<POOL, TA>(a, item, nwin, c, w, sc, sh);
    [[maybe_unused]] int pos0 = 0;
    [[maybe_unused]] uchar4 ar;
    [[maybe_unused]] float4 tg;
    if constexpr (TAP) {
      const unsigned tw = (unsigned)item / t.nbw;
      pos0 = (int)((unsigned)item - tw * t.nbw) * POOL;
      ar = *reinterpret_cast<const uchar4*>(t.arg + (long)tw * a.C + c);
      tg = ld4(t.dy + (long)tw * t.lddy + t.coff + c);
    }
#pragma unroll
    for (int j = 0; j < POOL; ++j) {
      if (j >= w.n) break;
      float4 o = bn_dx4(w.dz[j], w.v[j], mu, is, sc, k1, k2);
      am = amax4(am, o);
      if constexpr (TAP) {
        // the two steps this replaces, value for value: dx is stored (rounded to TA) and its word takes |dx|; then the
        // tap pass reads the stored element back, adds its gradient, stores again and merges |dx + g| into the word
        const int pj = pos0 + j;
        if (ar.x == pj) { o.x = add_unfused(round_act(dx, o.x), tg.x); am = fmaxf(am, fabsf(o.x)); }
        if (ar.y == pj) { o.y = add_unfused(round_act(dx, o.y), tg.y); am = fmaxf(am, fabsf(o.y)); }
        if (ar.z == pj) { o.z = add_unfused(round_act(dx, o.z), tg.z); am = fmaxf(am, fabsf(o.z)); }
        if (ar.w == pj) { o.w = add_unfused(round_act(dx, o.w), tg.w); am = fmaxf(am, fabsf(o.w)); }
      }
      st4(dx + (w.p0 + j) * a.C + c, o);
    }
  }
  amax_commit(am, amax);
}

template <int POOL, class TA>
__global__ __launch_bounds__(256) void bn_bwd_apply_win_kernel(const BnBwdArgsT<TA> a, long n_items, int nwin,
                                                               const float* __restrict__ c1,
                                                               const float* __restrict__ c2, TA* __restrict__ dx,
                                                               unsigned* __restrict__ amax) {
  bn_bwd_apply_win<POOL, TA>(a, n_items, nwin, c1, c2, dx, amax, NoTap{});
}

template <int POOL, class TA>
__global__ __launch_bounds__(256) void bn_bwd_apply_win_tap_kernel(const BnBwdArgsT<TA> a, long n_items, int nwin,
                                                                   const float* __restrict__ c1,
                                                                   const float* __restrict__ c2, TA* __restrict__ dx,
                                                                   unsigned* __restrict__ amax, const BnTapGrad<TA> t) {
  bn_bwd_apply_win<POOL, TA>(a, n_items, nwin, c1, c2, dx, amax, t);
}

// ---------------------------------------------------------------- plain MaxPool(1,k) (detector taps)
template <class TA>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const TA* __restrict__ x, TA* __restrict__ y,
                                                          long n_out_pix, int Fin, int C, int pool, long ldy,
                                                          int coff, unsigned char* __restrict__ arg) {
  // arg (optional, [n_out_pix][C] bytes): the window position of each maximum (first one wins, as torch's
  // max_pool2d backward routes it), so that the backward pass does not have to read x again
  const int quads = C >> 2, Fout = Fin / pool;
  const long total = n_out_pix * quads;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % quads);
    const long op = i / quads, row = op / Fout;
    const int fo = (int)(op % Fout);
    const TA* xp = x + ((row * Fin + (long)fo * pool) * C + q * 4);
    // FirstMax4::scan on variables of the kernel's own: with the maxima and positions in one struct the bf16 instance
    // comes out another kernel (42 -> 54 VGPRs, 604 -> 637 instructions), which has not been timed
    float4 m = ld4(xp);
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const auto take = [&](const float4& v, int pos) {
      first_max(m.x, a0, v.x, pos);
      first_max(m.y, a1, v.y, pos);
      first_max(m.z, a2, v.z, pos);
      first_max(m.w, a3, v.w, pos);
    };
    int j = 1;
    for (; j + 4 <= pool; j += 4) {                               // four window rows in flight
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld4(xp + (long)(j + u) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) take(v[u], j + u);
    }
    for (; j < pool; ++j) take(ld4(xp + (long)j * C), j);
    st4(y + op * ldy + coff + q * 4, m);
    if (arg != nullptr)
      *reinterpret_cast<uchar4*>(arg + op * C + q * 4) = make_uchar4((unsigned char)a0, (unsigned char)a1,
                                                                     (unsigned char)a2, (unsigned char)a3);
  }
}

// dx[first argmax of each window] += dy   (one thread owns a whole window: no atomics)
template <class TA>
__global__ __launch_bounds__(256) void maxpool_bwd_add_kernel(const TA* __restrict__ x,
                                                              const TA* __restrict__ dy, TA* __restrict__ dx,
                                                              long n_out_pix, int Fin, int C, int pool, long lddy,
                                                              int coff, unsigned* __restrict__ amax,
                                                              const unsigned char* __restrict__ arg) {
  // one thread per (window, channel quad): float4 loads, four window rows in flight, first maximum wins; with `arg`
  // (the positions maxpool_fwd_kernel recorded) x is not read at all
  const int Fout = Fin / pool, quads = C >> 2;
  const long total = n_out_pix * quads;
  float am = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long op = i / quads;
    const int c = (int)(i - op * quads) * 4;
    const long row = op / Fout;
    const int fo = (int)(op - row * Fout);
    int a0, a1, a2, a3;
    if (arg != nullptr) {
      const uchar4 a = *reinterpret_cast<const uchar4*>(arg + op * C + c);
      a0 = a.x; a1 = a.y; a2 = a.z; a3 = a.w;
    } else {
      const FirstMax4 m = FirstMax4::scan(x + (row * Fin + (long)fo * pool) * C + c, C, pool);
      a0 = m.p0; a1 = m.p1; a2 = m.p2; a3 = m.p3;
    }
    const float4 g = ld4(dy + op * lddy + coff + c);
    TA* dp = dx + (row * Fin + (long)fo * pool) * C + c;
    const float4 nv = make_float4(ld1(dp + (long)a0 * C) + g.x, ld1(dp + (long)a1 * C + 1) + g.y,
                                  ld1(dp + (long)a2 * C + 2) + g.z, ld1(dp + (long)a3 * C + 3) + g.w);
    st1(dp + (long)a0 * C, nv.x);
    st1(dp + (long)a1 * C + 1, nv.y);
    st1(dp + (long)a2 * C + 2, nv.z);
    st1(dp + (long)a3 * C + 3, nv.w);
    am = amax4(am, nv);          // merged into dx's word: an upper bound of max |dx| (elements that shrank keep their old share)
  }
  amax_commit(am, amax);
}

// ---------------------------------------------------------------- dropout (Philox4x32-10)
// rows x cols, x row stride ldx, y row stride ldy; mask is dense [rows*cols] bytes (1 = kept).
// mask_in != NULL replays a given mask (parity tests); otherwise keep = (u >= p).
template <class TA>
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const TA* __restrict__ x, long ldx,
                                                          TA* __restrict__ y, long ldy,
                                                          const uint8_t* __restrict__ mask_in,
                                                          uint8_t* __restrict__ mask_out, long rows, int cols,
                                                          float p, float scale, uint64_t seed, uint64_t offset) {
  const int quads = cols >> 2;
  const long total = rows * quads;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % quads) * 4;
    const long r = i / quads;
    uint8_t keep[4];
    if (mask_in) {
      const uchar4 m = *reinterpret_cast<const uchar4*>(mask_in + r * cols + c);
      keep[0] = m.x; keep[1] = m.y; keep[2] = m.z; keep[3] = m.w;
    } else {
      uint32_t rnd[4];
      philox4(seed, offset + (uint64_t)i, rnd);
#pragma unroll
      for (int k = 0; k < 4; ++k) keep[k] = ((float)(rnd[k] >> 8) * (1.0f / 16777216.0f)) >= p ? 1 : 0;
    }
    const float4 v = ld4(x + r * ldx + c);
    float4 o;
    o.x = keep[0] ? v.x * scale : 0.f;
    o.y = keep[1] ? v.y * scale : 0.f;
    o.z = keep[2] ? v.z * scale : 0.f;
    o.w = keep[3] ? v.w * scale : 0.f;
    st4(y + r * ldy + c, o);
    if (mask_out) *reinterpret_cast<uchar4*>(mask_out + r * cols + c) = make_uchar4(keep[0], keep[1], keep[2], keep[3]);
  }
}

// ---------------------------------------------------------------- (B,256,T,2) <-> (B,T,512) re-layout
// channels-last pixel pair (row, w in {0,1}) at x[(row*2 + w)*ldx + coff + c]  <->  seq[row][c*2 + w]
template <class TA>
__global__ __launch_bounds__(256) void nhwc_to_seq_kernel(const TA* __restrict__ x, long ldx, int coff,
                                                          float* __restrict__ seq, long rows, int C) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long r = i / C;
    const float a = ld1(x + (r * 2 + 0) * ldx + coff + c);
    const float b = ld1(x + (r * 2 + 1) * ldx + coff + c);
    *reinterpret_cast<float2*>(seq + r * 2 * C + 2 * c) = make_float2(a, b);
  }
}

template <class TA>
__global__ __launch_bounds__(256) void seq_to_nhwc_kernel(const float* __restrict__ seq, TA* __restrict__ x,
                                                          long ldx, int coff, long rows, int C, int accumulate) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long r = i / C;
    const float2 v = *reinterpret_cast<const float2*>(seq + r * 2 * C + 2 * c);
    TA* d0 = x + (r * 2 + 0) * ldx + coff + c;
    TA* d1 = x + (r * 2 + 1) * ldx + coff + c;
    if (accumulate) { st1(d0, ld1(d0) + v.x); st1(d1, ld1(d1) + v.y); }
    else { st1(d0, v.x); st1(d1, v.y); }
  }
}

// strided 2-D copy / add: dst[r*ldd + c] (+)= src[r*lds + c]
template <class TA>
__global__ __launch_bounds__(256) void copy2d_kernel(const TA* __restrict__ src, long lds, TA* __restrict__ dst,
                                                     long ldd, long rows, int cols, int accumulate) {
  const int quads = cols >> 2;
  const long total = rows * quads;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % quads) * 4;
    const long r = i / quads;
    float4 v = ld4(src + r * lds + c);
    TA* d = dst + r * ldd + c;
    if (accumulate) { const float4 o = ld4(d); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
    st4(d, v);
  }
}

int ew_grid(long total_threads) {
  long g = (total_threads + 255) / 256;
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return (int)g;
}

int reduce_grid(long n_pix, int C, int cap = 1024) {
  const int G = 256 / (C / 4);
  long g = (n_pix + G - 1) / G;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

size_t reduce_lds(int C) { return (size_t)(256 / (C / 4)) * 2 * C * sizeof(double); }

bool bn_channels_ok(int C) { return C >= 4 && (C % 4) == 0 && C <= 1024; }

// Calls fn(std::integral_constant<int, POOL>{}) for the pool widths the window-form kernels are built for (the ones
// JDCNet pools by) and returns its status; PE_E_UNSUPPORTED for any other (what with_act of forms.h is for `act16`).
template <class Fn>
int with_pool(int pool, Fn&& fn) {
  if (pool == 1) return fn(std::integral_constant<int, 1>{});
  if (pool == 2) return fn(std::integral_constant<int, 2>{});
  if (pool == 4) return fn(std::integral_constant<int, 4>{});
  return PE_E_UNSUPPORTED;
}

// ---------------------------------------------------------------- largest magnitude of a tensor (h2 operand scale)
// out[0] = max(out[0], IEEE bits of max |x|) over a row-strided [rows][cols] matrix (cols % 4 == 0).  The bit
// patterns of non-negative floats order like unsigned integers, so the cross-workgroup combine is an integer
// atomicMax: exact and independent of the order of arrival (NaN / inf operands give the largest patterns and poison
// the product they feed, as they would any other path).  The caller zeroes out[0] (pe_absmax does).
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long rows, int cols4, long ld,
                                                     unsigned* __restrict__ out) {
  const long n4 = rows * cols4;
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long r = i / cols4;
    const int c = (int)(i - r * cols4);
    const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c * 4);
    m = max(m, __float_as_uint(v.x) & 0x7fffffffu);
    m = max(m, __float_as_uint(v.y) & 0x7fffffffu);
    m = max(m, __float_as_uint(v.z) & 0x7fffffffu);
    m = max(m, __float_as_uint(v.w) & 0x7fffffffu);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  __shared__ unsigned red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, max(max(red[0], red[1]), max(red[2], red[3])));
}

// absmax of many segments of one buffer in a single launch (the model's parameters inside the flat buffer): block
// (x, y) folds chunk x of segment y and max-merges into out[y]
__global__ __launch_bounds__(256) void absmax_segments_kernel(const float* __restrict__ base,
                                                              const long* __restrict__ seg_off,
                                                              const long* __restrict__ seg_len,
                                                              unsigned* __restrict__ out) {
  const float* x = base + seg_off[blockIdx.y];
  const long n = seg_len[blockIdx.y];
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    m = max(m, __float_as_uint(x[i]) & 0x7fffffffu);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  __shared__ unsigned red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned w = max(max(red[0], red[1]), max(red[2], red[3]));
    if (w) atomicMax(out + blockIdx.y, w);
  }
}

}  // namespace

extern "C" size_t pe_bn_workspace_bytes(int C) { return (size_t)kMaxPartials * 2 * C * sizeof(double); }

template <class TA>
static int bn_train_stats_impl(const TA* x, long n_pix, int C, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !gamma || !beta || !mean || !invstd || !scale || !shift || n_pix <= 0) return PE_E_ARG;
  if (!bn_channels_ok(C)) return PE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < pe_bn_workspace_bytes(C)) return PE_E_WORKSPACE;
  hipStream_t st = pe_stream(stream);
  const int grid = reduce_grid(n_pix, C);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_stats_partial_kernel<TA>, dim3(grid), dim3(256), reduce_lds(C), st, x, n_pix, C, partial);
  PE_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(pe_cdiv(C, 4)), dim3(256), 0, st, partial, grid, n_pix, C, gamma,
                     beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_bn_train_stats(int act16, const void* x, long n_pix, int C, const float* gamma, const float* beta,
                                 float eps, float momentum, float* running_mean, float* running_var, float* mean,
                                 float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return bn_train_stats_impl(static_cast<const TA*>(x), n_pix, C, gamma, beta, eps, momentum, running_mean,
                               running_var, mean, invstd, scale, shift, workspace, workspace_bytes, stream);
  });
}

// BatchNorm training statistics from partials a producer kernel left behind ([nparts][2][C] doubles: column sums
// and sums of squares, e.g. pe_conv3x3_fwd_wf's bn_partials): the finalize half of pe_bn_train_stats.
extern "C" int pe_bn_finalize_stats(const double* partials, int nparts, long n_pix, int C, const float* gamma,
                                    const float* beta, float eps, float momentum, float* running_mean,
                                    float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!partials || !gamma || !beta || !mean || !invstd || !scale || !shift || n_pix <= 0 || nparts <= 0) return PE_E_ARG;
  if (!bn_channels_ok(C)) return PE_E_UNSUPPORTED;
  hipStream_t st = pe_stream(stream);
  const double* src = partials;
  int n = nparts;
  if (nparts > 512) {                    // fold tens of thousands of tile partials with coalesced reads first; the
    // per-thread chain is a serial sum, so the fold goes as wide as the finalize below still reads cheaply (30 k parts
    // over 128 blocks = 240 dependent adds per thread took 50 us per BatchNorm)
    constexpr int kFold = 512;
    if (!workspace || workspace_bytes < (size_t)kFold * 2 * C * sizeof(double)) return PE_E_WORKSPACE;
    double* folded = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(bn_partials_fold_kernel, dim3(kFold), dim3(256), 0, st, partials, nparts, 2 * C, folded);
    PE_LAUNCH_CHECK();
    src = folded;
    n = kFold;
  }
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(pe_cdiv(C, 4)), dim3(256), 0, st, src, n, n_pix, C, gamma, beta,
                     eps, momentum, running_mean, running_var, mean, invstd, scale, shift);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float eps, int C, float* scale, float* shift,
                                 float* mean, float* invstd, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || !mean || !invstd || C <= 0)
    return PE_E_ARG;
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(pe_cdiv(C, 64)), dim3(64), 0, pe_stream(stream), gamma, beta,
                     running_mean, running_var, eps, C, scale, shift, mean, invstd);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

template <class TA>
static int bn_act_pool_fwd_impl(const TA* x, const float* scale, const float* shift, float slope, TA* y, long rows,
                                int Fin, int C, int pool, long ldy, int coff, unsigned* amax_out, void* stream) {
  if (!x || !scale || !shift || !y || rows <= 0 || Fin <= 0 || pool <= 0) return PE_E_ARG;
  if (!bn_channels_ok(C) || (ldy & 3) || (coff & 3)) return PE_E_UNSUPPORTED;
  const long n_out = rows * (Fin / pool);
  hipLaunchKernelGGL(bn_act_pool_fwd_kernel<TA>, dim3(ew_grid(pe_cdiv(n_out, 256 / (C / 4)) * 256L)), dim3(256), 0, pe_stream(stream), x,
                     scale, shift, slope, y, n_out, Fin, C, pool, ldy, coff, amax_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_bn_act_pool_fwd(int act16, const void* x, const float* scale, const float* shift, float slope, void* y,
                                  long rows, int Fin, int C, int pool, long ldy, int coff, unsigned* amax_out,
                                  void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return bn_act_pool_fwd_impl(static_cast<const TA*>(x), scale, shift, slope, static_cast<TA*>(y), rows, Fin, C, pool,
                                ldy, coff, amax_out, stream);
  });
}

template <class TA>
static int bn_act_pool_bwd_impl(const TA* x, const TA* dy, const float* scale, const float* shift, const float* mean,
                                const float* invstd, float slope, TA* dx, float* dgamma, float* dbeta, long rows,
                                int Fin, int C, int pool, long lddy, int coff, int eval_mode, void* workspace,
                                size_t workspace_bytes, unsigned* amax_out, void* stream,
                                const BnTapGrad<TA>* tap = nullptr) {
  // eval_mode: mean / invstd are the running statistics the forward normalised with (pe_bn_eval_affine); dgamma and
  // dbeta may then be null together, and the per-channel reduction is not launched at all
  const bool sums = !(eval_mode && !dgamma && !dbeta);
  if (!x || !dy || !scale || !shift || !mean || !invstd || !dx || rows <= 0) return PE_E_ARG;
  if (sums && (!dgamma || !dbeta)) return PE_E_ARG;
  if (!bn_channels_ok(C) || (lddy & 3) || (coff & 3)) return PE_E_UNSUPPORTED;
  const size_t need = pe_bn_workspace_bytes(C) + 2 * (size_t)C * sizeof(float);
  if (sums && (!workspace || workspace_bytes < need)) return PE_E_WORKSPACE;
  hipStream_t st = pe_stream(stream);
  const BnBwdArgsT<TA> a{x, dy, scale, shift, mean, invstd, slope, rows * Fin, Fin, C, lddy, coff};
  double* partial = reinterpret_cast<double*>(workspace);
  float* c1 = eval_mode ? nullptr
                        : reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pe_bn_workspace_bytes(C));
  float* c2 = eval_mode ? nullptr : c1 + C;
  return with_pool(pool, [&](auto p) {
    constexpr int POOL = decltype(p)::value;
    const int nwin = Fin / POOL + (Fin % POOL ? 1 : 0);
    const long n_items = rows * nwin;
    if (sums) {
      // bf16 tensors without pooling: 8-byte requests, so four times the workgroups keep the same bytes in flight
      // (partial<1>: 348 -> 257 us; the pooled forms and fp32 tensors, at HBM speed with 1024, lose 5-10 % with more)
      const int grid = reduce_grid(n_items, C, (!std::is_same<TA, float>::value && POOL == 1) ? kMaxPartials : 1024);
      hipLaunchKernelGGL((bn_bwd_partial_win_kernel<POOL, TA>), dim3(grid), dim3(256), reduce_lds(C), st, a, n_items,
                         nwin, partial);
      PE_LAUNCH_CHECK();
      hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(pe_cdiv(C, 4)), dim3(256), 0, st, partial, grid, a.n_in_pix, C,
                         dgamma, dbeta, c1, c2);
      PE_LAUNCH_CHECK();
    }
    const dim3 agrid(ew_grid(pe_cdiv(n_items, 256 / (C / 4)) * 256L));
    if (tap != nullptr)
      hipLaunchKernelGGL((bn_bwd_apply_win_tap_kernel<POOL, TA>), agrid, dim3(256), 0, st, a, n_items, nwin, c1, c2, dx,
                         amax_out, *tap);
    else
      hipLaunchKernelGGL((bn_bwd_apply_win_kernel<POOL, TA>), agrid, dim3(256), 0, st, a, n_items, nwin, c1, c2, dx,
                         amax_out);
    PE_LAUNCH_CHECK();
    return (int)PE_OK;
  });
}

extern "C" int pe_bn_act_pool_bwd(int act16, const void* x, const void* dy, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, float slope, void* dx, float* dgamma,
                                  float* dbeta, long rows, int Fin, int C, int pool, long lddy, int coff, int eval_mode,
                                  void* workspace, size_t workspace_bytes, unsigned* amax_out, void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return bn_act_pool_bwd_impl(static_cast<const TA*>(x), static_cast<const TA*>(dy), scale, shift, mean, invstd, slope,
                                static_cast<TA*>(dx), dgamma, dbeta, rows, Fin, C, pool, lddy, coff, eval_mode,
                                workspace, workspace_bytes, amax_out, stream);
  });
}

// ---- detector tap folded into the BN passes (pe_bn_act_pool_tap_*)
// What the two tap kernels serve: whole tap windows made of whole BN windows, positions that fit a byte, and a tensor
// whose BN-window count fits the 32-bit division of the apply pass.
static bool tap_geometry_ok(long rows, int Fin, int C, int pool, int tap_pool, bool with_arg) {
  if (!bn_channels_ok(C) || rows <= 0 || Fin <= 0) return false;
  if (pool != 1 && pool != 2 && pool != 4) return false;
  if (tap_pool <= 0 || tap_pool % pool != 0 || Fin % tap_pool != 0) return false;
  if (with_arg && tap_pool > 255) return false;
  return rows * (long)Fin < (1L << 31);
}

extern "C" int pe_bn_act_pool_tap_supported(long rows, int Fin, int C, int pool, int tap_pool, int with_arg) {
  return tap_geometry_ok(rows, Fin, C, pool, tap_pool, with_arg != 0) ? 1 : 0;
}

template <class TA>
static int bn_act_pool_tap_fwd_impl(const TA* x, const float* scale, const float* shift, float slope, TA* y, long rows,
                                    int Fin, int C, int pool, long ldy, int coff, unsigned* amax_out, TA* tap_y,
                                    long tap_ldy, int tap_coff, int tap_pool, unsigned char* tap_arg, void* stream) {
  if (!x || !scale || !shift || !y || !tap_y || rows <= 0 || Fin <= 0 || pool <= 0) return PE_E_ARG;
  if ((ldy & 3) || (coff & 3) || (tap_ldy & 3) || (tap_coff & 3) ||
      !tap_geometry_ok(rows, Fin, C, pool, tap_pool, tap_arg != nullptr))
    return PE_E_UNSUPPORTED;
  const int G = 256 / (C / 4), nbw = tap_pool / pool;
  // segments per tap window: fill the pixel lanes (TW * S of G), then prefer the shorter segments
  int S = 1, used = 0;
  for (int s = 1; s <= G && s <= nbw; ++s) {
    if (nbw % s) continue;
    const int u = (G / s) * s;
    if (u >= used) { used = u; S = s; }
  }
  const long n_tap = rows * (Fin / tap_pool), n_trips = pe_cdiv(n_tap, (long)(G / S));
  const dim3 grid(ew_grid(n_trips * 256L));
  hipStream_t st = pe_stream(stream);
  return with_pool(pool, [&](auto p) {
    hipLaunchKernelGGL((bn_act_pool_tap_fwd_kernel<decltype(p)::value, TA>), grid, dim3(256), 0, st, x, scale, shift,
                       slope, y, n_tap, C, nbw, S, ldy, coff, amax_out, tap_y, tap_ldy, tap_coff, tap_arg);
    PE_LAUNCH_CHECK();
    return (int)PE_OK;
  });
}

extern "C" int pe_bn_act_pool_tap_fwd(int act16, const void* x, const float* scale, const float* shift, float slope,
                                      void* y, long rows, int Fin, int C, int pool, long ldy, int coff,
                                      unsigned* amax_out, void* tap_y, long tap_ldy, int tap_coff, int tap_pool,
                                      unsigned char* tap_arg, void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return bn_act_pool_tap_fwd_impl(static_cast<const TA*>(x), scale, shift, slope, static_cast<TA*>(y), rows, Fin, C,
                                    pool, ldy, coff, amax_out, static_cast<TA*>(tap_y), tap_ldy, tap_coff, tap_pool,
                                    tap_arg, stream);
  });
}

extern "C" int pe_bn_act_pool_tap_bwd(int act16, const void* x, const void* dy, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, float slope, void* dx, float* dgamma,
                                      float* dbeta, long rows, int Fin, int C, int pool, long lddy, int coff,
                                      int eval_mode, void* workspace, size_t workspace_bytes, unsigned* amax_out,
                                      const void* tap_dy,
                                      long tap_lddy, int tap_coff, int tap_pool, const unsigned char* tap_arg,
                                      void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    if (!tap_dy || !tap_arg) return (int)PE_E_ARG;
    if ((tap_lddy & 3) || (tap_coff & 3) || !tap_geometry_ok(rows, Fin, C, pool, tap_pool, true))
      return (int)PE_E_UNSUPPORTED;
    const BnTapGrad<TA> tap{static_cast<const TA*>(tap_dy), tap_arg, tap_lddy, tap_coff, (unsigned)(tap_pool / pool)};
    return bn_act_pool_bwd_impl(static_cast<const TA*>(x), static_cast<const TA*>(dy), scale, shift, mean, invstd, slope,
                                static_cast<TA*>(dx), dgamma, dbeta, rows, Fin, C, pool, lddy, coff, eval_mode,
                                workspace, workspace_bytes, amax_out, stream, &tap);
  });
}

template <class TA>
static int maxpool_fwd_impl(const TA* x, TA* y, long rows, int Fin, int C, int pool, long ldy, int coff,
                            unsigned char* argmax_out, void* stream) {
  if (!x || !y || rows <= 0 || Fin <= 0 || pool <= 0) return PE_E_ARG;
  if ((C & 3) || (ldy & 3) || (coff & 3) || (argmax_out && pool > 255)) return PE_E_UNSUPPORTED;
  const long n_out = rows * (Fin / pool);
  hipLaunchKernelGGL(maxpool_fwd_kernel<TA>, dim3(ew_grid(n_out * (C / 4))), dim3(256), 0, pe_stream(stream), x, y,
                     n_out, Fin, C, pool, ldy, coff, argmax_out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_maxpool_fwd(int act16, const void* x, void* y, long rows, int Fin, int C, int pool, long ldy, int coff,
                              unsigned char* argmax_out, void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return maxpool_fwd_impl(static_cast<const TA*>(x), static_cast<TA*>(y), rows, Fin, C, pool, ldy, coff, argmax_out,
                            stream);
  });
}

template <class TA>
static int maxpool_bwd_add_impl(const TA* x, const unsigned char* argmax, const TA* dy, TA* dx, long rows, int Fin,
                                int C, int pool, long lddy, int coff, unsigned* amax_out, void* stream) {
  if ((!x && !argmax) || !dy || !dx || rows <= 0 || Fin <= 0 || pool <= 0 || C <= 0) return PE_E_ARG;
  if ((C & 3) || (lddy & 3) || (coff & 3)) return PE_E_UNSUPPORTED;
  const long n_out = rows * (Fin / pool);
  hipLaunchKernelGGL(maxpool_bwd_add_kernel<TA>, dim3(ew_grid(n_out * (C / 4))), dim3(256), 0, pe_stream(stream), x,
                     dy, dx, n_out, Fin, C, pool, lddy, coff, amax_out, argmax);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_maxpool_bwd_add(int act16, const void* x, const unsigned char* argmax, const void* dy, void* dx,
                                  long rows, int Fin, int C, int pool, long lddy, int coff, unsigned* amax_out,
                                  void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return maxpool_bwd_add_impl(static_cast<const TA*>(x), argmax, static_cast<const TA*>(dy), static_cast<TA*>(dx),
                                rows, Fin, C, pool, lddy, coff, amax_out, stream);
  });
}

template <class TA>
static int dropout_fwd_impl(const TA* x, long ldx, TA* y, long ldy, const unsigned char* mask_in,
                            unsigned char* mask_out, long rows, int cols, float p, unsigned long long seed,
                            unsigned long long offset, void* stream) {
  if (!x || !y || rows <= 0 || cols <= 0 || p < 0.f || p >= 1.f) return PE_E_ARG;
  if ((cols & 3) || (ldx & 3) || (ldy & 3)) return PE_E_UNSUPPORTED;
  hipLaunchKernelGGL(dropout_fwd_kernel<TA>, dim3(ew_grid(rows * (cols / 4))), dim3(256), 0, pe_stream(stream), x, ldx,
                     y, ldy, mask_in, mask_out, rows, cols, p, 1.0f / (1.0f - p), (uint64_t)seed, (uint64_t)offset);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_dropout_fwd(int act16, const void* x, long ldx, void* y, long ldy, const unsigned char* mask_in,
                              unsigned char* mask_out, long rows, int cols, float p, unsigned long long seed,
                              unsigned long long offset, void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return dropout_fwd_impl(static_cast<const TA*>(x), ldx, static_cast<TA*>(y), ldy, mask_in, mask_out, rows, cols, p,
                            seed, offset, stream);
  });
}

template <class TA>
static int nhwc_to_seq_impl(const TA* x, long ldx, int coff, float* seq, long rows, int C, void* stream) {
  if (!x || !seq || rows <= 0 || C <= 0) return PE_E_ARG;
  hipLaunchKernelGGL(nhwc_to_seq_kernel<TA>, dim3(ew_grid(rows * C)), dim3(256), 0, pe_stream(stream), x, ldx, coff, seq,
                     rows, C);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_nhwc_to_seq(int act16, const void* x, long ldx, int coff, float* seq, long rows, int C, void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return nhwc_to_seq_impl(static_cast<const TA*>(x), ldx, coff, seq, rows, C, stream);
  });
}

template <class TA>
static int seq_to_nhwc_impl(const float* seq, TA* x, long ldx, int coff, long rows, int C, int accumulate, void* stream) {
  if (!x || !seq || rows <= 0 || C <= 0) return PE_E_ARG;
  hipLaunchKernelGGL(seq_to_nhwc_kernel<TA>, dim3(ew_grid(rows * C)), dim3(256), 0, pe_stream(stream), seq, x, ldx, coff,
                     rows, C, accumulate);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_seq_to_nhwc(int act16, const float* seq, void* x, long ldx, int coff, long rows, int C, int accumulate,
                              void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return seq_to_nhwc_impl(seq, static_cast<TA*>(x), ldx, coff, rows, C, accumulate, stream);
  });
}

template <class TA>
static int copy2d_impl(const TA* src, long lds, TA* dst, long ldd, long rows, int cols, int accumulate, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0) return PE_E_ARG;
  if ((cols & 3) || (lds & 3) || (ldd & 3)) return PE_E_UNSUPPORTED;
  hipLaunchKernelGGL(copy2d_kernel<TA>, dim3(ew_grid(rows * (cols / 4))), dim3(256), 0, pe_stream(stream), src, lds, dst,
                     ldd, rows, cols, accumulate);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_copy2d(int act16, const void* src, long lds, void* dst, long ldd, long rows, int cols, int accumulate,
                         void* stream) {
  return with_act(act16, [&](auto a) {
    using TA = typename decltype(a)::TA;
    return copy2d_impl(static_cast<const TA*>(src), lds, static_cast<TA*>(dst), ldd, rows, cols, accumulate, stream);
  });
}

extern "C" int pe_absmax(const float* x, long rows, int cols, long ld, unsigned* out, void* stream) {
  if (!x || !out || rows < 0 || cols <= 0 || ld < cols) return PE_E_ARG;
  if ((cols & 3) || (ld & 3) || (reinterpret_cast<uintptr_t>(x) & 15)) return PE_E_UNSUPPORTED;
  hipStream_t st = pe_stream(stream);
  PE_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(unsigned), st));
  if (rows == 0) return PE_OK;
  const long n4 = rows * (cols / 4);
  const int grid = (int)(n4 / 2048 < 1 ? 1 : n4 / 2048 > 2048 ? 2048 : n4 / 2048);     // >= 8 float4 per thread
  hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, st, x, rows, cols / 4, ld, out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

extern "C" int pe_absmax_segments(const float* base, const long* seg_off, const long* seg_len, int nseg, unsigned* out,
                                  void* stream) {
  if (!base || !seg_off || !seg_len || !out || nseg <= 0 || nseg > 65535) return PE_E_ARG;
  hipStream_t st = pe_stream(stream);
  PE_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)nseg * sizeof(unsigned), st));
  hipLaunchKernelGGL(absmax_segments_kernel, dim3(16, nseg), dim3(256), 0, st, base, seg_off, seg_len, out);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
