// Activation element access for the two storage formats of the conv stack's tensors: fp32 (parity path) and bf16
// (mixed precision: what the reference's autocast keeps in memory for conv / linear outputs, trainer.py:226-235 and
// README.md:36 -- half the HBM bytes of every BatchNorm / pooling / staging pass and half the saved-for-backward
// footprint).  Arithmetic is always fp32: ld4 widens (a 16-bit shift), st4 rounds to nearest even.
#pragma once
#include "common.h"

namespace pe {

typedef __bf16 act16_t;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }

__device__ __forceinline__ float4 ld4(const act16_t* p) {            // 4 consecutive bf16 (8-byte aligned)
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float4 ld4(const _Float16* p) {           // 4 consecutive fp16 (8-byte aligned)
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 v = *reinterpret_cast<const h4*>(p);
  return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
__device__ __forceinline__ unsigned pack_bf16_rne(float a, float b) {
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}
__device__ __forceinline__ void st4(act16_t* p, const float4& v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16_rne(v.x, v.y), pack_bf16_rne(v.z, v.w));
}
__device__ __forceinline__ float ld1(const act16_t* p) {
  return __uint_as_float((unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
}
__device__ __forceinline__ void st1(act16_t* p, float v) { *p = (act16_t)v; }

// A quad as it comes out of memory: kernels keep the loaded bits in registers until they are staged (converting right
// after the load would put the conversion -- and with it the wait for the load -- in front of the MFMA phase the load
// is meant to overlap: the bf16-tensor weight-gradient kernel ran 2x slower that way).
template <class T> struct RawQuad;
template <> struct RawQuad<float> { typedef float4 type; };
template <> struct RawQuad<act16_t> { typedef uint2 type; };
__device__ __forceinline__ float4 ldraw(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint2 ldraw(const act16_t* p) { return *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ float4 widen(const float4& v) { return v; }
__device__ __forceinline__ float4 widen(const uint2& u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
// the same quad through a buffer descriptor: voffset / soffset in bytes, out-of-range requests read as zero
template <class T> __device__ __forceinline__ typename RawQuad<T>::type ldraw_buffer(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff);
template <> __device__ __forceinline__ float4 ldraw_buffer<float>(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  const u4 d = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return make_float4(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z), __uint_as_float(d.w));
}
template <> __device__ __forceinline__ uint2 ldraw_buffer<act16_t>(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  const u2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
  return make_uint2(d.x, d.y);
}
// One output element / quad through a buffer descriptor (epilogues): `voff` in bytes, a request past the descriptor's
// range reads zero / is dropped, so a tile's overhang costs no branch.  Same bytes as ld1 / st1 / st4.
// (a load comes back in its storage form; widen1 at the point of use keeps the wait for it out of the issue phase)
__device__ __forceinline__ unsigned ld1raw_buffer(const float*, __amdgpu_buffer_rsrc_t rs, unsigned voff) {
  return __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0);
}
__device__ __forceinline__ unsigned ld1raw_buffer(const act16_t*, __amdgpu_buffer_rsrc_t rs, unsigned voff) {
  return (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs, voff, 0, 0);
}
__device__ __forceinline__ float widen1(const float*, unsigned raw) { return __uint_as_float(raw); }
__device__ __forceinline__ float widen1(const act16_t*, unsigned raw) { return __uint_as_float(raw << 16); }
__device__ __forceinline__ void st1_buffer(float*, __amdgpu_buffer_rsrc_t rs, unsigned voff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, voff, 0, 0);
}
__device__ __forceinline__ void st1_buffer(act16_t*, __amdgpu_buffer_rsrc_t rs, unsigned voff, float v) {
  __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (act16_t)v), rs, voff, 0, 0);
}
__device__ __forceinline__ void st4_buffer(float*, __amdgpu_buffer_rsrc_t rs, unsigned voff, const float4& v) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  const u4 d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(d, rs, voff, 0, 0);
}
__device__ __forceinline__ void st4_buffer(act16_t*, __amdgpu_buffer_rsrc_t rs, unsigned voff, const float4& v) {
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  const u2 d = {pack_bf16_rne(v.x, v.y), pack_bf16_rne(v.z, v.w)};
  __builtin_amdgcn_raw_buffer_store_b64(d, rs, voff, 0, 0);
}
// Offsets of such a descriptor are 32 bits with bit 31 as the "outside" marker: it serves tensors below 2 GiB.
constexpr unsigned kBufferOutside = 0x80000000u;

template <class R> __device__ __forceinline__ R zero_raw();
template <> __device__ __forceinline__ float4 zero_raw<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ uint2 zero_raw<uint2>() { return make_uint2(0u, 0u); }

}  // namespace pe
