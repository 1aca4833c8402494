// Split-K skeleton of the weight-gradient products (pe_gemm_tn, pe_lstm_whh_grad, pe_conv3x3_wgrad): a long reduction
// dimension K (batch x time, or pixels) is cut into k-splits of whole k-tiles, each (split, tile) workgroup writes its
// fp32 partial tile into the slab of its split, and one reduce kernel sums the slabs in double, in split order -- the
// result does not depend on the order the workgroups ran in.  A plan of one split stores to the destination directly.
//
// Here: the plan, the workspace bound, the (split, tile) decode of a workgroup, the TN kernel and its launcher, and
// the reduce.  A caller supplies its tile, its loaders and two numbers: the shortest k-split worth a workgroup and
// the number of workgroups the chip holds at once.
#pragma once
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

// C[m][n] = sum_k A[k][m] . B[k][n] over this workgroup's k-split, operands through the TN loaders AL / BL
template <int BM, int BN, int MODE, class AL, class BL, class TH>
__global__ __launch_bounds__(256) void tn_splitk_kernel(AL al, BL bl, float* out, long ldo, long split_stride, int M,
                                                        int N, int K, int k_per_split, int tiles_n, int accumulate,
                                                        const unsigned* amax_a, const unsigned* amax_b) {
  __shared__ __attribute__((aligned(16))) float As[tn_lds_floats<MODE, BM>()];
  __shared__ __attribute__((aligned(16))) float Bs[tn_lds_floats<MODE, BN>()];
  const SplitKBlock b = splitk_block<BM, BN>((M + BM - 1) / BM, tiles_n, K, k_per_split);
  al.init(b.m0, b.kb);
  bl.init(b.n0, b.kb);
  f32x16 acc[BM / 64][BN / 64];
  tn_zero_acc<BM, BN>(acc);
  H2Scales hs{1.f, 1.f, 1.f};
  if constexpr (MODE == kSplit2) hs.load(amax_a, amax_b);
  tn_mainloop_mode<MODE, BM, BN, 1, TH>(al, bl, b.kb, b.ke, As, Bs, acc, hs.sa, hs.sb);
  float* dst = out + (long)b.split_id * split_stride;
  tn_for_each_acc<BM, BN>(acc, [&](int r, int c, float v) {
    const int row = b.m0 + r, col = b.n0 + c;
    if constexpr (MODE == kSplit2) v = hs.unscale(v);
    if (row < M && col < N) {
      float* d = dst + (long)row * ldo + col;
      if (accumulate) v += *d;
      *d = v;
    }
  });
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
// and the reduce.  C may be an unaligned view (scalar stores on both paths).
template <int BM, int BN, class F, class AL, class BL>
int launch_tn(const AL& al, const BL& bl, float* C, long ldc, int M, int N, int K, int accumulate, float* ws,
              size_t ws_bytes, hipStream_t st, const unsigned* amax_a, const unsigned* amax_b) {
  constexpr int MODE = F::MODE;
  const int tm = pe_cdiv(M, BM), tn = pe_cdiv(N, BN);
  const SplitK p = splitk_plan(tm * tn, K, kTnMinKps, tn_resident(MODE));
  auto kernel = tn_splitk_kernel<BM, BN, MODE, AL, BL, typename F::TH>;
  if (p.splits == 1) {
    hipLaunchKernelGGL(kernel, dim3(tm * tn), dim3(256), 0, st, al, bl, C, ldc, 0L, M, N, K, p.kps, tn, accumulate,
                       amax_a, amax_b);
    PE_LAUNCH_CHECK();
    return PE_OK;
  }
  if (!ws || ws_bytes < (size_t)p.splits * M * N * sizeof(float)) return PE_E_WORKSPACE;
  hipLaunchKernelGGL(kernel, dim3(tm * tn * p.splits), dim3(256), 0, st, al, bl, ws, (long)N, (long)M * N, M, N, K,
                     p.kps, tn, 0, amax_a, amax_b);
  PE_LAUNCH_CHECK();
  return launch_splitk_reduce(ws, p.splits, RowMajorDst{C, ldc, M, N, accumulate}, st);
}

}  // namespace
}  // namespace pe
