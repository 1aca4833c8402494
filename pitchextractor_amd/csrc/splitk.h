// Split-K skeleton of the weight-gradient products (pe_gemm_tn, pe_lstm_whh_grad, pe_conv3x3_wgrad): a long reduction
// dimension K (batch x time, or pixels) is cut into k-splits of whole k-tiles, each (split, tile) workgroup writes its
// fp32 partial tile into the slab of its split, and one reduce kernel sums the slabs in double, in split order -- the
// result does not depend on the order the workgroups ran in.  A plan of one split stores to the destination directly.
//
// Here: the plan, the workspace bound, the (split, tile) decode of a workgroup, the TN kernel and its launcher, and
// the reduce.  A caller supplies its tile, its loaders and two numbers: the shortest k-split worth a workgroup and
// the number of workgroups the chip holds at once.
#pragma once
#include <initializer_list>
#include "forms.h"

namespace pe {

// ------------------------------------------------------------------ plan
struct SplitK { int splits, kps; };                        // kps: k per split, a multiple of kBK

constexpr int resident_wgs(int per_cu) { return 256 * per_cu; }
// The TN engine runs 3 workgroups per CU, 2 when the LDS holds multi-term images (bf16 / f16: one small image, 3 too)
constexpr int tn_resident(int mode) { return resident_wgs(mode == kSplit || mode == kSplit2 ? 2 : 3); }
constexpr int kTnMinKps = 512;                             // shortest k-split of pe_gemm_tn / pe_lstm_whh_grad

static inline SplitK splitk_plan(int tiles, int K, int min_kps, int resident) {
  const int s = pe_pick_splits(tiles, K, min_kps, resident);
  const int kps = pe_cdiv(pe_cdiv(K, s), kBK) * kBK;
  return {pe_cdiv(K, kps), kps};
}

// Most splits any form of a TN entry point plans (forms differ by tn_resident alone): sizes the one workspace that
// serves them all.
static inline int tn_max_splits(int tiles, int K) {
  const int a = splitk_plan(tiles, K, kTnMinKps, tn_resident(kNative)).splits;
  const int b = splitk_plan(tiles, K, kTnMinKps, tn_resident(kSplit)).splits;
  return a > b ? a : b;
}

// ------------------------------------------------------------------ tile of a product planned on 128 x 128
// The 192-wide tiles stage fewer operand elements per MFMA (per k-tile 128 x 128: 96 MFMAs for 8 192 staged elements,
// 128 x 192: 144 for 10 240, 192 x 192: 216 for 12 288).  A form has a tile when its term images fit the 64 KB of static
// LDS: h2 and the one-term forms have all of them, x3 (three images per operand) and the native loop none.
template <int MODE, int BM, int BN> constexpr bool tn_tile_fits() {
  return (BM <= 128 && BN <= 128) ||
         (MODE != kNative && (tn_lds_floats<MODE, BM>() + tn_lds_floats<MODE, BN>()) * sizeof(float) <= 65536);
}
// BM * 1000 + BN: the override (PE_TN_TILE), else the first of `preferred` (the wide tiles an entry point measured
// faster than 128 x 128, best first) whose tiling pads M x N to no more area than the 128 x 128 one, else 128 x 128
static inline int tn_tile_for(int M, int N, std::initializer_list<int> preferred) {
  if (const int o = pe_tn_tile_override()) return o;
  const long base = pe_cdiv(M, 128) * 128L * pe_cdiv(N, 128) * 128L;
  for (const int t : preferred) {
    const long bm = t / 1000, bn = t % 1000;
    if (pe_cdiv(M, bm) * bm * pe_cdiv(N, bn) * bn <= base) return t;
  }
  return 128128;
}

// ------------------------------------------------------------------ (split, tile) of a workgroup
struct SplitKBlock { int m0, n0, kb, ke, split_id; };

// 1-D grid over (split, tile) with every XCD taking a CONTIGUOUS run of it: the tiles of one k-split then share
// an XCD's L2 for the operand rows they all read (PMC: 2.3 GB of fabric reads per dW_ih launch, 5x the operands,
// with the (tile, split) grid whose consecutive workgroups go round-robin over the eight XCDs)
template <int BM, int BN>
__device__ __forceinline__ SplitKBlock splitk_block(int tiles_m, int tiles_n, int K, int kps) {
  const int tiles_mn = tiles_m * tiles_n;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);                // grid = tiles_mn * splits workgroups
  const int tile_id = lin % tiles_mn, split_id = lin / tiles_mn;
  const int m0 = (tile_id / tiles_n) * BM, n0 = (tile_id % tiles_n) * BN;
  const int kb = split_id * kps;
  const int ke = min(K, kb + kps);
  return {m0, n0, kb, ke, split_id};
}

// ------------------------------------------------------------------ reduce destinations
struct RowMajorDst {                                       // C[M][N] with leading dimension ldc (N % 4 == 0)
  float* C;
  long ldc;
  int M, N, accumulate;
  __host__ __device__ long elems() const { return (long)M * N; }
  __device__ __forceinline__ void operator()(long i4, const float4& s) const {
    const long idx = i4 * 4;
    const int row = (int)(idx / N), col = (int)(idx - (long)row * N);
    float* d = C + (long)row * ldc + col;                          // C may be an unaligned view: scalar stores
    if (accumulate) { d[0] += s.x; d[1] += s.y; d[2] += s.z; d[3] += s.w; }
    else { d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w; }
  }
};

namespace {   // kernels and their launchers: every translation unit that includes this file owns its instances

// Workgroups per CU asked of the compiler: the 192-wide tiles hold up to 144 accumulator registers per lane and are
// meant to run two to a CU (their LDS allows no more); the narrower instances keep the default bound.
template <int BM, int BN> constexpr int tn_min_blocks() { return BM == 192 || BN == 192 ? 2 : 1; }

// C[m][n] = sum_k A[k][m] . B[k][n] over this workgroup's k-split, operands through the TN loaders AL / BL.
// The 16-bit-term modes run the main loop with the operand roles swapped (gemm_engine.h, tn_mainloop_split SW: the
// same bits), so a lane owns column quads of one row and the tile leaves in 16-byte pieces.  BUF: the pieces go
// through a buffer descriptor that covers exactly the rows below M of this slab / destination; a row past M lies
// past its range by itself (ldo >= N), a column quad past N is sent there (kBufferOutside), and the stores are
// dropped without a branch.  Needs accumulate == 0, a 16-byte aligned `out`, ldo % 4 == 0 and N % 4 == 0, and
// (M + BM) * ldo * 4 below 2 GiB (checked by launch_tn).  !BUF is the pointer form with scalar stores: unaligned
// views, accumulating launches, outputs of 2 GiB and more, PE_EPILOGUE=pointer, and the native fp32 loop.
template <int BM, int BN, int MODE, bool BUF, class AL, class BL, class TH>
__global__ __launch_bounds__(256, (tn_min_blocks<BM, BN>()))
void tn_splitk_kernel(AL al, BL bl, float* out, long ldo, long split_stride, int M, int N, int K, int k_per_split,
                      int tiles_n, int accumulate, const unsigned* amax_a, const unsigned* amax_b) {
  constexpr bool SW = MODE != kNative;
  static_assert(SW || !BUF, "the native fp32 loop keeps the scalar epilogue");
  __shared__ __attribute__((aligned(16))) float As[tn_lds_floats<MODE, BM>()];
  __shared__ __attribute__((aligned(16))) float Bs[tn_lds_floats<MODE, BN>()];
  static_assert((tn_lds_floats<MODE, BM>() + tn_lds_floats<MODE, BN>()) * sizeof(float) <= 65536, "static LDS");
  const SplitKBlock b = splitk_block<BM, BN>((M + BM - 1) / BM, tiles_n, K, k_per_split);
  al.init(b.m0, b.kb);
  bl.init(b.n0, b.kb);
  f32x16 acc[BM / 64][BN / 64];
  tn_zero_acc<BM, BN>(acc);
  H2Scales hs{1.f, 1.f, 1.f};
  if constexpr (MODE == kSplit2) hs.load(amax_a, amax_b);
  tn_mainloop_mode<MODE, BM, BN, 1, TH, SW>(al, bl, b.kb, b.ke, As, Bs, acc, hs.sa, hs.sb);
  float* dst = out + (long)b.split_id * split_stride;
  auto element = [&](int row, int col, float v) {
    if (row < M && col < N) {
      float* d = dst + (long)row * ldo + col;
      if (accumulate) v += *d;
      *d = v;
    }
  };
  if constexpr (!SW) {
    tn_for_each_acc<BM, BN>(acc, [&](int r, int c, float v) { element(b.m0 + r, b.n0 + c, v); });
  } else {
    auto unscale4 = [&](float4 v) {
      if constexpr (MODE == kSplit2) {
        v.x = hs.unscale(v.x); v.y = hs.unscale(v.y); v.z = hs.unscale(v.z); v.w = hs.unscale(v.w);
      }
      return v;
    };
    if constexpr (BUF) {
      const unsigned rowb = (unsigned)ldo * 4u;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          dst, 0, (unsigned)(((long)(M - 1) * ldo + N) * (long)sizeof(float)), 0x00020000);
      tn_for_each_quad<BM, BN>(acc, [&](int r, int c, const float4& v) {
        const int col = b.n0 + c;
        st4_buffer(dst, rs, col < N ? (unsigned)(b.m0 + r) * rowb + (unsigned)col * 4u : kBufferOutside, unscale4(v));
      });
    } else {
      tn_for_each_quad<BM, BN>(acc, [&](int r, int c, const float4& q) {
        const float4 v = unscale4(q);
        const int row = b.m0 + r, col = b.n0 + c;
        element(row, col, v.x); element(row, col + 1, v.y); element(row, col + 2, v.z); element(row, col + 3, v.w);
      });
    }
  }
}

// dst(i4, sum over the slabs of float4 i4), slabs summed in split order
template <class Dst>
__global__ void splitk_reduce_kernel(const float* ws, long split_stride, int splits, Dst dst) {
  const long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 * 4 >= dst.elems()) return;
  dst(i4, pe_ordered_slab_sum4(ws, split_stride, splits, i4));
}

template <class Dst>
int launch_splitk_reduce(const float* ws, int splits, const Dst& dst, hipStream_t st) {
  const long n = dst.elems();                                      // = the slab stride
  hipLaunchKernelGGL(splitk_reduce_kernel<Dst>, dim3(pe_cdiv(n / 4, 256)), dim3(256), 0, st, ws, n, splits, dst);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

// C[M][N] (+)= A^T B with a BM x BN tile: one launch storing to C when the plan has one split, else slabs in `ws`
// and the reduce.  C may be an unaligned view (then scalar stores on both paths).
//
// PM x PN is the tile the split-K PLAN is made for -- the tile the entry point's workspace query counts with -- and
// BM x BN the tile a workgroup computes.  A wider BM x BN changes the grid and the tile decode only: splits, kps, slab
// stride, workspace bytes and the reduce launch are those of the PM x PN tiling, and the result has the same bits:
//   - each k-split covers the same rows [split * kps, min(K, (split + 1) * kps)), in k-tiles of 32 from its first row;
//   - an output element's sum over a k-split is one MFMA accumulator chain in k order, and which k go to which MFMA
//     (the k-slot map of the fragments) does not depend on where the element's 32 x 32 block sits in a tile, nor on
//     the tile's size;
//   - splitk_reduce_kernel sums the same slabs in the same order.
//
// A 192-wide tile exists in the buffer form only (its pointer form would not fit 256 registers without scratch): where
// a launch needs the pointer form, launch_tn of such a tile launches nothing and returns kTnNarrowTile, and the caller
// runs the PM x PN tile.
constexpr int kTnNarrowTile = -1000;                       // internal: never leaves an entry point

template <int BM, int BN, class F, int PM = BM, int PN = BN, class AL, class BL>
int launch_tn(const AL& al, const BL& bl, float* C, long ldc, int M, int N, int K, int accumulate, float* ws,
              size_t ws_bytes, hipStream_t st, const unsigned* amax_a, const unsigned* amax_b) {
  constexpr int MODE = F::MODE;
  constexpr bool WIDE = BM > 128 || BN > 128;
  static_assert(!WIDE || MODE != kNative, "the native fp32 loop has no 192-wide tile");
  const int tm = pe_cdiv(M, BM), tn = pe_cdiv(N, BN);
  const SplitK p = splitk_plan(pe_cdiv(M, PM) * pe_cdiv(N, PN), K, kTnMinKps, tn_resident(MODE));
  auto buffer = tn_splitk_kernel<BM, BN, MODE, MODE != kNative, AL, BL, typename F::TH>;
  auto pointer = tn_splitk_kernel<BM, BN, MODE, WIDE, AL, BL, typename F::TH>;      // (WIDE: not launched)
  // the 16-byte pieces through a buffer descriptor (tn_splitk_kernel, BUF): its 32-bit offsets must also hold the
  // rows a tile hangs over M by
  auto quads = [&](const float* out, long ldo) {
    return MODE != kNative && (N & 3) == 0 && (ldo & 3) == 0 && ldo >= N &&
           (reinterpret_cast<uintptr_t>(out) & 15) == 0 && pe_epilogue_buffer((long)(M + BM) * ldo * (long)sizeof(float));
  };
  const bool direct = p.splits == 1;
  const bool buf = direct ? !accumulate && quads(C, ldc) : quads(ws, N);
  if (WIDE && !buf) return kTnNarrowTile;
  if (direct) {
    hipLaunchKernelGGL(buf ? buffer : pointer, dim3(tm * tn), dim3(256), 0, st, al, bl, C, ldc, 0L, M, N, K, p.kps, tn,
                       accumulate, amax_a, amax_b);
    PE_LAUNCH_CHECK();
    return PE_OK;
  }
  if (!ws || ws_bytes < (size_t)p.splits * M * N * sizeof(float)) return PE_E_WORKSPACE;
  hipLaunchKernelGGL(buf ? buffer : pointer, dim3(tm * tn * p.splits), dim3(256), 0, st, al, bl, ws, (long)N,
                     (long)M * N, M, N, K, p.kps, tn, 0, amax_a, amax_b);
  PE_LAUNCH_CHECK();
  return launch_splitk_reduce(ws, p.splits, RowMajorDst{C, ldc, M, N, accumulate}, st);
}

}  // namespace
}  // namespace pe
