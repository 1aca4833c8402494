// Stitching the model's chunk outputs into rows (inference.predict_f0_batch): the valid frames of every chunk back to
// back ("concat"), every frame from the chunk it lies most centrally in ("center"), or the two chunks of a seam
// cross-faded ("crossfade").  The host describes a call as runs of consecutive frames (include/pitchextractor_hip.h);
// the kernel walks the DESTINATION, so every output element is written once -- a copy, a blend or a zero -- by one
// launch whatever the number of rows.
//
// Work split: a frame of C columns is cut into ceil(C / 4) slots of four columns and a thread takes one slot of one
// frame.  A full slot whose source and destination addresses are 16-byte aligned moves as one float4 (global_load /
// store_dwordx4: 1 KiB per wave instruction, the width the memory pipe wants); any other slot -- C = 1, the last slot
// of an odd C, a packed row that starts at an odd element, every second frame of C = 722 -- moves column by column.
// Consecutive lanes take consecutive slots of a frame, so a wave's accesses are contiguous within a frame.  The run of
// a frame is found by a binary search of the run table (sorted by destination; a few KiB, served from L2).  No LDS,
// 34 VGPRs, 8 waves per SIMD.  The traffic is one read and one write of the logits.
// A variant that searched once per four consecutive frames, issued their loads before the first store and moved
// 8-byte-aligned slots as two float2 measured the same on an MI355X (722 columns: 61.0 against 59.9 us, DESIGN.md
// section 17), so the search chain is not what bounds the kernel and the simpler form stays.
#include "common.h"

namespace {

enum { R_A = 0, R_FA, R_DST, R_LEN, R_NOV, R_J0, R_B, R_FB, R_K };

constexpr int kThreads = 256;

struct StitchArgs {
  const float* x;
  long ld_x;
  const float* det;
  const long* runs;
  int n_runs, chunk_size, C, slots;
  float* out;
  long ld_out;
  float* det_out;
  long n_dst;
};

__global__ __launch_bounds__(kThreads) void stitch_chunks_kernel(const StitchArgs a) {
  const long total = a.n_dst * a.slots;
  const long step = (long)gridDim.x * kThreads;
  for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < total; g += step) {
    const long d = g / a.slots;
    const int c0 = 4 * (int)(g - d * a.slots);
    const int nc = min(4, a.C - c0);
    // the last run that starts at or before d
    int lo = 0, hi = a.n_runs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.runs[(long)mid * R_K + R_DST] <= d) lo = mid + 1; else hi = mid;
    }
    float* dst = a.out + d * a.ld_out + c0;
    const long* run = a.runs + (long)(lo - 1) * R_K;
    const long i = lo > 0 ? d - run[R_DST] : 0;
    if (lo == 0 || i >= run[R_LEN]) {                      // no run covers this frame
      for (int c = 0; c < nc; ++c) dst[c] = 0.0f;
      if (a.det_out && c0 == 0) a.det_out[d] = 0.0f;
      continue;
    }
    const long fa = run[R_A] * a.chunk_size + run[R_FA] + i;
    const float* pa = a.x + fa * a.ld_x + c0;
    const long n_ov = run[R_NOV];
    if (n_ov == 0) {
      if (nc == 4 && ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(pa);
      } else {
        for (int c = 0; c < nc; ++c) dst[c] = pa[c];
      }
      if (a.det_out && c0 == 0) a.det_out[d] = a.det[fa];
      continue;
    }
    const long fb = run[R_B] * a.chunk_size + run[R_FB] + i;
    const float* pb = a.x + fb * a.ld_x + c0;
    const float w = (float)(run[R_J0] + i + 1) / (float)(n_ov + 1);
    if (nc == 4 && ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb) |
                     reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
      const float4 va = *reinterpret_cast<const float4*>(pa), vb = *reinterpret_cast<const float4*>(pb);
      *reinterpret_cast<float4*>(dst) = make_float4(va.x + w * (vb.x - va.x), va.y + w * (vb.y - va.y),
                                                    va.z + w * (vb.z - va.z), va.w + w * (vb.w - va.w));
    } else {
      for (int c = 0; c < nc; ++c) dst[c] = pa[c] + w * (pb[c] - pa[c]);
    }
    if (a.det_out && c0 == 0) a.det_out[d] = a.det[fa] + w * (a.det[fb] - a.det[fa]);
  }
}

int stitch_cus() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
              ? prop.multiProcessorCount : 256;
  }
  return cus;
}

}  // namespace

extern "C" int pe_stitch_run_fields(void) { return R_K; }

extern "C" int pe_stitch_chunks(const float* x, long ld_x, const float* det, const long* runs, const long* host_runs,
                                int n_runs, int n_chunks, int chunk_size, int C, float* out, long ld_out,
                                float* det_out, long n_dst, void* stream) {
  if (n_runs < 0 || n_chunks < 0 || chunk_size < 0 || n_dst < 0) return PE_E_ARG;
  if (C < 1 || C > 1024) return PE_E_UNSUPPORTED;
  if (ld_x < C || ld_out < C || (det == nullptr) != (det_out == nullptr)) return PE_E_ARG;
  if (n_runs > 0 && !host_runs) return PE_E_ARG;
  long next = 0;                                           // first destination frame a run may still take
  for (int r = 0; r < n_runs; ++r) {
    const long* m = host_runs + (long)r * R_K;
    if (m[R_LEN] < 1 || m[R_DST] < next || m[R_DST] > n_dst - m[R_LEN]) return PE_E_ARG;
    if (m[R_A] < 0 || m[R_A] >= n_chunks || m[R_FA] < 0 || m[R_FA] > chunk_size - m[R_LEN]) return PE_E_ARG;
    if (m[R_NOV] < 0 || m[R_NOV] >= (1L << 24)) return PE_E_ARG;
    if (m[R_NOV] > 0 && (m[R_B] < 0 || m[R_B] >= n_chunks || m[R_FB] < 0 || m[R_FB] > chunk_size - m[R_LEN] ||
                         m[R_J0] < 0 || m[R_J0] > m[R_NOV] - m[R_LEN])) return PE_E_ARG;
    next = m[R_DST] + m[R_LEN];
  }
  if (n_dst == 0) return PE_OK;
  if (!out || (n_runs > 0 && (!x || !runs))) return PE_E_ARG;

  StitchArgs a;
  a.x = x; a.ld_x = ld_x; a.det = det; a.runs = runs; a.n_runs = n_runs; a.chunk_size = chunk_size; a.C = C;
  a.slots = (C + 3) / 4; a.out = out; a.ld_out = ld_out; a.det_out = det_out; a.n_dst = n_dst;
  const long blocks = (n_dst * a.slots + kThreads - 1) / kThreads;
  const long resident = (long)stitch_cus() * 8;            // 8 workgroups of 4 waves per CU: 8 waves per SIMD
  hipLaunchKernelGGL(stitch_chunks_kernel, dim3((unsigned)(blocks < resident ? blocks : resident)), dim3(kThreads), 0,
                     pe_stream(stream), a);
  PE_LAUNCH_CHECK();
  return PE_OK;
}
