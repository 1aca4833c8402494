// Dense fp32 GEMMs on the MFMA tile engines (gemm_engine.h).
//
//   pe_gemm_nt:  C[M][N] = A[M][K] . B[N][K]^T (+ bias0[n] + bias1[n]) (+ C)
//                -> nn.Linear forward, LSTM input projections (model.py:220-227), 1x1 convs in
//                   channels-last (model.py:53,167), transposed-weight dgrad products.
//   pe_gemm_tn:  C[M][N] = sum_k A[k][m] . B[k][n]  (k = rows), split over k across workgroups
//                -> weight gradients (dW = dY^T X), deterministic slab + ordered reduce.
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include "splitk.h"


namespace {
using namespace pe;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class TO>
struct StoreEpiT {
  TO* C;
  long ldc;
  const float* bias0;
  const float* bias1;
  int M, N, accumulate;
  __device__ __forceinline__ void operator()(int row, int col, float v) const {
    if (row < M && col < N) {
      if (bias0) v += bias0[col];
      if (bias1) v += bias1[col];
      TO* dst = C + (long)row * ldc + col;
      if (accumulate) v += ld1(dst);
      st1(dst, v);
    }
  }
};
typedef StoreEpiT<float> StoreEpi;

template <class TL, int MODE, class TA = float, class TH = __bf16>
__global__ __launch_bounds__(256) void gemm_nt_kernel(RowLoaderT<TA> al, RowLoader bl, StoreEpiT<TA> ep, int K,
                                                      int tiles_m, int tiles_n, const unsigned* amax_a,
                                                      const unsigned* amax_b) {
  __shared__ __attribute__((aligned(16))) float As[TL::BM * nt_row_floats<MODE>()];
  __shared__ __attribute__((aligned(16))) float Bs[TL::BN * nt_row_floats<MODE>()];
  const int tile = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int m0 = (tile / tiles_n) * TL::BM, n0 = (tile % tiles_n) * TL::BN;
  al.init(m0);
  bl.init(n0);
  f32x16 acc[TL::TM][TL::TN];
  zero_acc<TL>(acc);
  H2Scales hs{1.f, 1.f, 1.f};
  if constexpr (MODE == kSplit2) hs.load(amax_a, amax_b);
  nt_mainloop_mode<TL, MODE, false, 1, TH>(al, bl, K, As, Bs, acc, hs.sa, hs.sb);
  for_each_acc<TL>(acc, [&](int r, int c, float v) { ep(m0 + r, n0 + c, MODE == kSplit2 ? hs.unscale(v) : v); });
}

// The same product with the operand roles swapped inside the tile engine (the NT main loop is symmetric in its two
// operands): the accumulators then hold the TRANSPOSED 32 x 32 blocks, i.e. a lane owns four consecutive output
// columns of one row instead of four rows of one column, and the epilogue writes 16-byte pieces (a quarter of the
// store instructions, bias fetched once per column quad).  Bit-identical sums.  Needs N % 4 == 0 and a 16-byte
// aligned C with ldc % 4 == 0 (checked by the host).
// BUF picks the epilogue at compile time (with both in one kernel hipcc reads every accumulator out of the AGPRs in
// front of the choice, which costs the 128 x 128 and 256 x 64 instances their third workgroup per CU).
// Three workgroups per CU is what the 128 x 128 and 256 x 64 main loops fit (all but the x3 256 x 64 one); the bound
// keeps the epilogue's loads in flight from taking a register or two more than that allows.
template <class TL, int MODE> constexpr int nt_t_min_blocks() {
  return TL::BM * TL::BN == 128 * 128 && !(MODE == kSplit && TL::BM == 256) ? 3 : 1;
}
template <class TL, int MODE, bool BUF, class TA = float, class TH = __bf16>
__global__ __launch_bounds__(256, (nt_t_min_blocks<TL, MODE>()))
void gemm_nt_t_kernel(RowLoaderT<TA> al, RowLoader bl, StoreEpiT<TA> ep, int K, int tiles_m, int tiles_n,
                      const unsigned* amax_a, const unsigned* amax_b) {
  using TT = Tile<TL::BN, TL::BM, TL::WAVES_N, TL::WAVES_M>;
  __shared__ __attribute__((aligned(16))) float As[TL::BM * nt_row_floats<MODE>()];
  __shared__ __attribute__((aligned(16))) float Bs[TL::BN * nt_row_floats<MODE>()];
  const int tile = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int m0 = (tile / tiles_n) * TL::BM, n0 = (tile % tiles_n) * TL::BN;
  al.init(m0);
  bl.init(n0);
  f32x16 acc[TT::TM][TT::TN];
  zero_acc<TT>(acc);
  H2Scales hs{1.f, 1.f, 1.f};
  if constexpr (MODE == kSplit2) hs.load(amax_a, amax_b);
  nt_mainloop_mode<TT, MODE, true, 1, TH>(bl, al, K, Bs, As, acc, hs.sb, hs.sa);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wn = wv / TT::WAVES_N, wm = wv % TT::WAVES_N;          // TT's "rows" are output columns
  const int r = lane & 31, h = lane >> 5;
  // A lane's quads: group (i, q) = output columns n0 + wn WM + 32 i + 8 q + 4 h .. + 3, rows m0 + wm WN + 32 j + r.
  auto quad = [&](int i, int q, int j) {
    float4 v = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
    if constexpr (MODE == kSplit2) {
      v.x = hs.unscale(v.x); v.y = hs.unscale(v.y); v.z = hs.unscale(v.z); v.w = hs.unscale(v.w);
    }
    return v;
  };
  auto add4 = [](float4& v, const float4& o) { v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; };
  if constexpr (BUF) {
    // Buffer form (C ends below 2 GiB): C and the biases go through buffer descriptors.  C's covers the rows below M
    // exactly, so a row past M lies past its range by itself; a column quad past N is sent there (kBufferOutside):
    // loads read zero, stores are dropped, no branch per quad -- and the guard columns of an ldc > N view are never
    // touched, because quads are whole (N % 4 == 0).  The old values of an accumulate launch and the bias quads are
    // requested one group ahead of their use and waited for once per group, not once per load.
    // Order of the sums as in the scalar epilogue: ((acc + bias0) + bias1) + old.
    typedef typename RawQuad<TA>::type Raw;
    const unsigned esz = (unsigned)sizeof(TA), rowb = (unsigned)ep.ldc * esz;
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
        ep.C, 0, (unsigned)(((long)(ep.M - 1) * ep.ldc + ep.N) * (long)sizeof(TA)), 0x00020000);
    const unsigned nbytes = (unsigned)ep.N * 4u;
    const __amdgpu_buffer_rsrc_t b0rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ep.bias0), 0, ep.bias0 ? nbytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t b1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ep.bias1), 0, ep.bias1 ? nbytes : 0u, 0x00020000);
    const unsigned rowo = (unsigned)(m0 + wm * TT::WN + r) * rowb;
    constexpr int G = TT::TM * 4;
    auto col_of = [&](int g) { return n0 + wn * TT::WM + (g >> 2) * 32 + 8 * (g & 3) + 4 * h; };
    auto voff = [&](int g, int j) {
      const int col = col_of(g);
      return (col < ep.N ? rowo + (unsigned)col * esz : kBufferOutside) + (unsigned)(j * 32) * rowb;
    };
    // An absent bias adds -0.0f, which changes no value (the biases' uniform choice without a branch per group);
    // accumulate picks one of two straight-line copies.
    const float4 nz = make_float4(-0.f, -0.f, -0.f, -0.f);
    const bool has0 = ep.bias0 != nullptr, has1 = ep.bias1 != nullptr;
    auto run = [&](auto acc_tag) {
      constexpr bool ACC = decltype(acc_tag)::value;
      Raw old[2][TT::TN];
      float4 b0[2], b1[2];
      auto fetch = [&](int g) {
        const int col = col_of(g);
        const unsigned bo = col < ep.N ? (unsigned)col * 4u : kBufferOutside;
        b0[g & 1] = ldraw_buffer<float>(b0rs, bo, 0u);             // (a null bias: an empty descriptor, nothing is read)
        b1[g & 1] = ldraw_buffer<float>(b1rs, bo, 0u);
        if constexpr (ACC) {
#pragma unroll
          for (int j = 0; j < TT::TN; ++j) old[g & 1][j] = ldraw_buffer<TA>(crs, voff(g, j), 0u);
        }
      };
      fetch(0);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g + 1 < G) fetch(g + 1);
        __builtin_amdgcn_sched_barrier(0);                         // keep the next group's loads in front of the stores
        const float4 c0 = has0 ? b0[g & 1] : nz, c1 = has1 ? b1[g & 1] : nz;
#pragma unroll
        for (int j = 0; j < TT::TN; ++j) {
          float4 v = quad(g >> 2, g & 3, j);
          add4(v, c0);
          add4(v, c1);
          if constexpr (ACC) add4(v, widen(old[g & 1][j]));
          st4_buffer(ep.C, crs, voff(g, j), v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (ep.accumulate) run(std::true_type{});
    else run(std::false_type{});
  } else {                                                         // pointer form: C past 2 GiB, PE_EPILOGUE=pointer
#pragma unroll
    for (int i = 0; i < TT::TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = n0 + wn * TT::WM + i * 32 + 8 * q + 4 * h;
        if (col >= ep.N) continue;
        float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;        // (acc + bias0) + bias1, as the scalar epilogue
        if (ep.bias0) b0 = make_float4(ep.bias0[col], ep.bias0[col + 1], ep.bias0[col + 2], ep.bias0[col + 3]);
        if (ep.bias1) b1 = make_float4(ep.bias1[col], ep.bias1[col + 1], ep.bias1[col + 2], ep.bias1[col + 3]);
#pragma unroll
        for (int j = 0; j < TT::TN; ++j) {
          const int row = m0 + wm * TT::WN + j * 32 + r;
          if (row >= ep.M) continue;
          TA* dst = ep.C + (long)row * ep.ldc + col;
          float4 v = quad(i, q, j);
          if (ep.bias0) add4(v, b0);
          if (ep.bias1) add4(v, b1);
          if (ep.accumulate) add4(v, ld4(dst));
          st4(dst, v);
        }
      }
  }
}

template <class TL, class F, class TA = typename F::TA>
int launch_nt(const RowLoaderT<TA>& al, const RowLoader& bl, const StoreEpiT<TA>& ep, int M, int N, int K,
              hipStream_t st, const unsigned* amax_a, const unsigned* amax_b) {
  constexpr int MODE = F::MODE;
  using TH = typename F::TH;
  const int tm = pe_cdiv(M, TL::BM), tn = pe_cdiv(N, TL::BN);
  const bool vec = MODE != kNative && (N & 3) == 0 && (ep.ldc & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(ep.C) & (4 * sizeof(TA) - 1)) == 0;
  if (vec) {
    // buffer form: the descriptor's 32-bit offsets must also hold the rows a tile hangs over M by
    if (ep.ldc >= N && pe_epilogue_buffer((long)(M + TL::BM) * ep.ldc * (long)sizeof(TA)))
      hipLaunchKernelGGL((gemm_nt_t_kernel<TL, MODE, true, TA, TH>), dim3(tm * tn), dim3(256), 0, st, al, bl, ep, K, tm,
                         tn, amax_a, amax_b);
    else
      hipLaunchKernelGGL((gemm_nt_t_kernel<TL, MODE, false, TA, TH>), dim3(tm * tn), dim3(256), 0, st, al, bl, ep, K, tm,
                         tn, amax_a, amax_b);
  }
  else
    hipLaunchKernelGGL((gemm_nt_kernel<TL, MODE, TA, TH>), dim3(tm * tn), dim3(256), 0, st, al, bl, ep, K, tm, tn, amax_a,
                       amax_b);
  PE_LAUNCH_CHECK();
  return PE_OK;
}

}  // namespace

template <class F, class TA = typename F::TA>
static int gemm_nt_impl(const TA* A, long lda, const float* B, long ldb, TA* C, long ldc, int M, int N,
                        int K, const float* bias0, const float* bias1, int accumulate, void* stream,
                        const unsigned* amax_a, const unsigned* amax_b) {
  constexpr int MODE = F::MODE;
  if (!A || !B || !C || M < 0 || N < 0 || K <= 0) return PE_E_ARG;
  if (MODE == kSplit2 && (!amax_a || !amax_b)) return PE_E_ARG;
  if (M == 0 || N == 0) return PE_OK;
  if ((K & 3) || (lda & 3) || (ldb & 3) || (reinterpret_cast<uintptr_t>(A) & (4 * sizeof(TA) - 1)) || !aligned16(B))
    return PE_E_UNSUPPORTED;
  // the operand loaders address a tile's rows through 32-bit buffer offsets (gemm_engine.h, RowLoaderT)
  if (lda < 0 || ldb < 0 || lda >= (1L << 21) || ldb >= (1L << 21)) return PE_E_UNSUPPORTED;
  RowLoaderT<TA> al{A, lda, M, K, 0};
  RowLoader bl{B, ldb, N, K, 0};
  StoreEpiT<TA> ep{C, ldc, bias0, bias1, M, N, accumulate};
  hipStream_t st = pe_stream(stream);
  if (N <= 32) return launch_nt<Tile<128, 32, 4, 1>, F>(al, bl, ep, M, N, K, st, amax_a, amax_b);
  if (N <= 64) return launch_nt<Tile<256, 64, 4, 1>, F>(al, bl, ep, M, N, K, st, amax_a, amax_b);
  if (N % 192 == 0 && (N % 128 != 0 || MODE != kNative))   // 16-bit-term modes: the wider tile stages 17 % fewer rows per MFMA
    return launch_nt<Tile<128, 192, 2, 2>, F>(al, bl, ep, M, N, K, st, amax_a, amax_b);
  return launch_nt<Tile<128, 128, 2, 2>, F>(al, bl, ep, M, N, K, st, amax_a, amax_b);
}

extern "C" int pe_gemm_nt(int products, int act16, const void* A, long lda, const float* B, long ldb, void* C, long ldc,
                          int M, int N, int K, const float* bias0, const float* bias1, int accumulate,
                          const unsigned* amax_a, const unsigned* amax_b, void* stream) {
  // act16: bf16 ACTIVATION STORAGE, A and C are bf16 tensors in HBM (weights and biases stay fp32)
  return with_form<kAllForms, true>(products, act16, [&](auto f) {
    using TA = typename decltype(f)::TA;
    return gemm_nt_impl<decltype(f)>(static_cast<const TA*>(A), lda, B, ldb, static_cast<TA*>(C), ldc, M, N, K, bias0,
                                     bias1, accumulate, stream, amax_a, amax_b);
  });
}

extern "C" size_t pe_gemm_tn_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int s = tn_max_splits(pe_cdiv(M, M <= 64 ? 64 : 128) * pe_cdiv(N, N <= 64 ? 64 : 128), K);
  return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;            // one split stores to C directly
}

template <class F, class TA = typename F::TA>
static int gemm_tn_impl(const TA* A, long lda, const TA* B, long ldb, float* C, long ldc, int M, int N,
                        int K, int accumulate, float* workspace, size_t workspace_bytes, void* stream,
                        const unsigned* amax_a, const unsigned* amax_b) {
  constexpr int MODE = F::MODE;
  if (!A || !B || !C || M < 0 || N < 0 || K <= 0) return PE_E_ARG;
  if (MODE == kSplit2 && (!amax_a || !amax_b)) return PE_E_ARG;
  if (M == 0 || N == 0) return PE_OK;
  if ((M & 3) || (N & 3) || (lda & 3) || (ldb & 3) || (reinterpret_cast<uintptr_t>(A) & (4 * sizeof(TA) - 1)) ||
      (reinterpret_cast<uintptr_t>(B) & (4 * sizeof(TA) - 1)))
    return PE_E_UNSUPPORTED;
  if (lda < 0 || ldb < 0 || lda >= (1L << 24) || ldb >= (1L << 24)) return PE_E_UNSUPPORTED;   // 32-bit offsets per k-tile
  hipStream_t st = pe_stream(stream);
  auto launch = [&](auto bm, auto bn) {
    constexpr int BM = decltype(bm)::value, BN = decltype(bn)::value;
    // (the plan is that of pe_gemm_tn_workspace_bytes: a 192-wide tile runs the k-splits of the 128-wide tiling)
    return launch_tn<BM, BN, F, (BM < 128 ? BM : 128), (BN < 128 ? BN : 128)>(
        KRowLoader<BM, TA>{A, lda, M, 0}, KRowLoader<BN, TA>{B, ldb, N, 0}, C, ldc, M, N, K, accumulate, workspace,
        workspace_bytes, st, amax_a, amax_b);
  };
  std::integral_constant<int, 64> t64;
  std::integral_constant<int, 128> t128;
  std::integral_constant<int, 192> t192;
  if (M <= 64 && N <= 64) return launch(t64, t64);
  if (M <= 64) return launch(t64, t128);
  if (N <= 64) return launch(t128, t64);
  // Shapes planned on 128 x 128: the first 192-wide tile that pads M x N no further, in the order measured on the
  // step's shapes (profiles/ab_tn_tile.txt: 1536 x 768 on 192 x 192, 1536 x 512 and 192 x 128 on 192 x 128, 256 x 192
  // on 128 x 192 are 4-21 % faster in h2; 256 x 640, which every wide tile pads further, is 15-35 % slower on them)
  const int tile = tn_tile_for(M, N, {192192, 192128, 128192});
  int rc = kTnNarrowTile;                                          // (what a wide tile answers that cannot serve the launch)
  if constexpr (tn_tile_fits<MODE, 192, 192>())
    if (tile == 192192) rc = launch(t192, t192);
  if constexpr (tn_tile_fits<MODE, 192, 128>())
    if (tile == 192128) rc = launch(t192, t128);
  if constexpr (tn_tile_fits<MODE, 128, 192>())
    if (tile == 128192) rc = launch(t128, t192);
  return rc != kTnNarrowTile ? rc : launch(t128, t128);
}

extern "C" int pe_gemm_tn(int products, int act16, const void* A, long lda, const void* B, long ldb, float* C, long ldc,
                          int M, int N, int K, int accumulate, float* workspace, size_t workspace_bytes,
                          const unsigned* amax_a, const unsigned* amax_b, void* stream) {
  return with_form<kAllForms, true>(products, act16, [&](auto f) {   // act16: A and B are bf16 tensors in HBM
    using TA = typename decltype(f)::TA;
    return gemm_tn_impl<decltype(f)>(static_cast<const TA*>(A), lda, static_cast<const TA*>(B), ldb, C, ldc, M, N, K,
                                     accumulate, workspace, workspace_bytes, stream, amax_a, amax_b);
  });
}
