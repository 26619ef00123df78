// The two tensor conversions around the depth network (include/dmslam_depthnet.h; DepthPrediction::predict,
// GUI/src/Tools/DepthPrediction.cpp:106-169): interleaved RGB8 -> [1, 3, H, W] of byte * (1/255), and [1, 1, H, W] metres -> u16 mm.
//
// Both are pure streaming over 0.3 - 1.8 M elements, so the work is in the memory shape:
//   * a lane owns one GROUP of consecutive pixels sized so that what it writes to a plane is one 16-byte store (4 fp32 or 8 fp16
//     values for pack, 8 u16 for unpack); a wave's store instruction then covers 1 KiB of contiguous memory;
//   * the groups start at the first element whose OUTPUT address is a multiple of 16; the elements before it (the head, fewer than a
//     group) and after the last whole group (the tail) are written one by one, by the first lanes of the grid, in the same launch;
//   * the group's input is read once, with the widest loads its address allows: 16-byte loads when the first group's input is
//     16-byte aligned (then every group's is), else dword loads, else byte (pack) / halfword (fp16 unpack) loads of the same bytes;
//   * pack's three planes are width * height elements apart: they share their alignment only when that is a multiple of 16 bytes
//     (every camera size with width * height a multiple of 4 / 8, 640 x 480 and 1241 x 376 among them).  Otherwise no group size
//     aligns all three and the element-wise kernel runs (4- / 2-byte stores, still coalesced);
//   * grid-stride loop, no LDS, nothing kept between launches.
// The arithmetic is written with __fmul_rn / rintf so that no contraction or reassociation can touch it (and the library is built with
// -ffp-contract=off -fno-fast-math): one IEEE multiply and one rounding, the same sequence as tests/depthnet_ref.py.
#include <hip/hip_fp16.h>

#include "../../include/dmslam_depthnet.h"
#include "common.hpp"

namespace dms {
namespace {

constexpr int kMaxStreamBlocks = 2048;  // 8 blocks of 256 threads per CU; the grid-stride loop takes the rest

// ---- the arithmetic ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float unit_of_byte(unsigned b) { return __fmul_rn((float)b, (float)(1.0 / 255.0)); }
__device__ __forceinline__ unsigned half_bits(float v) { return (unsigned)__half_as_ushort(__float2half_rn(v)); }
__device__ __forceinline__ float half_value(unsigned bits) { return __half2float(__ushort_as_half((unsigned short)bits)); }

__device__ __forceinline__ unsigned millimetres(float x, int mode) {
  const float r = __fmul_rn(x, 1000.0f);
  if (mode == DMS_DEPTHNET_TRUNCATE) {
    const float c = fminf(fmaxf(r, 0.0f), 65535.0f);  // (NaN: selected away below)
    return r != r ? 0u : (unsigned)(int)c;              // the C conversion truncates
  }
  const float v = rintf(r);  // nearest, ties to even
  const float c = fminf(fmaxf(v, 0.0f), 65535.0f);
  return v < 2147483648.0f ? (unsigned)(int)c : 0u;  // false for NaN, +inf and v >= 2^31; v <= -2^31 (-inf too) saturates to the same 0
}

// ---- loads of a group's input: NW dwords at p, which is aligned to ALIGN bytes ---------------------------------------------
template <int NW, int ALIGN>
__device__ __forceinline__ void load_words(const unsigned char* p, uint32_t (&w)[NW]) {
  if constexpr (ALIGN == 16) {
    static_assert(NW % 4 == 0, "whole 16-byte loads");
#pragma unroll
    for (int k = 0; k < NW / 4; ++k) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[k];
      w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
  } else if constexpr (ALIGN == 4) {
    struct __attribute__((packed, aligned(4))) Words {
      uint32_t w[NW];
    };
    const Words v = *reinterpret_cast<const Words*>(p);
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = v.w[k];
  } else if constexpr (ALIGN == 2) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const unsigned short* h = reinterpret_cast<const unsigned short*>(p) + 2 * k;
      w[k] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NW; ++k)
      w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
  }
}
__device__ __forceinline__ unsigned byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// ---- pack ------------------------------------------------------------------------------------------------------------------
template <bool HALF>
__device__ __forceinline__ void pack_one(const unsigned char* rgb, int channels, void* out, size_t n, size_t i) {
  const unsigned char* px = rgb + i * (size_t)channels;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = unit_of_byte(px[c]);
    if constexpr (HALF)
      reinterpret_cast<unsigned short*>(out)[(size_t)c * n + i] = (unsigned short)half_bits(v);
    else
      reinterpret_cast<float*>(out)[(size_t)c * n + i] = v;
  }
}

// planes with a common alignment: `head` pixels one by one, `groups` groups of G pixels from pixel `head` on, then the tail
template <int C, bool HALF, int ALIGN>
__global__ __launch_bounds__(kBlock) void k_depthnet_pack(const unsigned char* __restrict__ rgb, void* __restrict__ out, unsigned n, unsigned head,
                                                         unsigned groups) {
  constexpr int G = HALF ? 8 : 4;    // pixels per group: 16 bytes of each plane
  constexpr int NW = G * C / 4;      // dwords of input per group
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned body_end = head + groups * (unsigned)G;  // <= n
  const unsigned edge = head + (n - body_end);             // < 2 G
  if (gid < edge) pack_one<HALF>(rgb, C, out, n, gid < head ? gid : body_end + (gid - head));
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned g = gid; g < groups; g += stride) {
    const size_t i0 = (size_t)head + (size_t)g * G;
    uint32_t w[NW];
    load_words<NW, ALIGN>(rgb + i0 * C, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[G];
#pragma unroll
      for (int k = 0; k < G; ++k) v[k] = unit_of_byte(byte_of(w, k * C + c));
      if constexpr (HALF) {
        uint4 o;
        o.x = half_bits(v[0]) | (half_bits(v[1]) << 16);
        o.y = half_bits(v[2]) | (half_bits(v[3]) << 16);
        o.z = half_bits(v[4]) | (half_bits(v[5]) << 16);
        o.w = half_bits(v[6]) | (half_bits(v[7]) << 16);
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(out) + (size_t)c * n + i0) = o;
      } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + (size_t)c * n + i0) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

// planes that do not share their alignment: one pixel per lane and step
template <bool HALF>
__global__ __launch_bounds__(kBlock) void k_depthnet_pack_elementwise(const unsigned char* __restrict__ rgb, int channels, void* __restrict__ out,
                                                                     unsigned n) {
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pack_one<HALF>(rgb, channels, out, n, i);
}

// ---- unpack ----------------------------------------------------------------------------------------------------------------
template <bool HALF>
__device__ __forceinline__ void unpack_one(const void* in, unsigned short* depth, size_t i, int mode) {
  const float x = HALF ? half_value(reinterpret_cast<const unsigned short*>(in)[i]) : reinterpret_cast<const float*>(in)[i];
  depth[i] = (unsigned short)millimetres(x, mode);
}

template <bool HALF, int ALIGN>
__global__ __launch_bounds__(kBlock) void k_depthnet_unpack(const void* __restrict__ in, unsigned short* __restrict__ depth, unsigned n, unsigned head,
                                                           unsigned groups, int mode) {
  constexpr int G = 8;                // 8 u16 = one 16-byte store
  constexpr int NW = HALF ? 4 : 8;    // dwords of input per group
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned body_end = head + groups * (unsigned)G;
  const unsigned edge = head + (n - body_end);
  if (gid < edge) unpack_one<HALF>(in, depth, gid < head ? gid : body_end + (gid - head), mode);
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned g = gid; g < groups; g += stride) {
    const size_t i0 = (size_t)head + (size_t)g * G;
    uint32_t w[NW];
    load_words<NW, ALIGN>(reinterpret_cast<const unsigned char*>(in) + i0 * (HALF ? 2 : 4), w);
    unsigned mm[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      float x;
      if constexpr (HALF)
        x = half_value((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
      else
        x = __uint_as_float(w[k]);
      mm[k] = millimetres(x, mode);
    }
    uint4 o;
    o.x = mm[0] | (mm[1] << 16), o.y = mm[2] | (mm[3] << 16), o.z = mm[4] | (mm[5] << 16), o.w = mm[6] | (mm[7] << 16);
    *reinterpret_cast<uint4*>(depth + i0) = o;
  }
}

// the split of n elements of `elem` bytes at `out` into head / groups of G / tail, groups starting at the first 16-byte boundary
inline void split(const void* out, unsigned n, int elem, int G, unsigned* head, unsigned* groups) {
  const unsigned mis = (unsigned)((uintptr_t)out & 15u);
  unsigned h = mis ? (16u - mis) / (unsigned)elem : 0u;
  if (h > n) h = n;
  *head = h;
  *groups = (n - h) / (unsigned)G;
}
inline unsigned stream_blocks(unsigned lanes) {
  const unsigned b = (lanes + kBlock - 1) / kBlock;
  return b < 1 ? 1 : (b > (unsigned)kMaxStreamBlocks ? (unsigned)kMaxStreamBlocks : b);
}

template <int C, bool HALF>
void launch_pack(const unsigned char* rgb, void* out, unsigned n, unsigned head, unsigned groups, hipStream_t s) {
  constexpr int G = HALF ? 8 : 4;
  const unsigned lanes = groups > 2u * G ? groups : 2u * G;
  const dim3 grid(stream_blocks(lanes)), block(kBlock);
  const uintptr_t first = (uintptr_t)(rgb + (size_t)head * C);
  if (C == 4 && (first & 15u) == 0)
    hipLaunchKernelGGL((k_depthnet_pack<C, HALF, C == 4 ? 16 : 4>), grid, block, 0, s, rgb, out, n, head, groups);
  else if ((first & 3u) == 0)
    hipLaunchKernelGGL((k_depthnet_pack<C, HALF, 4>), grid, block, 0, s, rgb, out, n, head, groups);
  else
    hipLaunchKernelGGL((k_depthnet_pack<C, HALF, 1>), grid, block, 0, s, rgb, out, n, head, groups);
}

template <bool HALF>
void launch_unpack(const void* in, unsigned short* depth, unsigned n, int mode, hipStream_t s) {
  unsigned head, groups;
  split(depth, n, 2, 8, &head, &groups);
  const unsigned lanes = groups > 16u ? groups : 16u;
  const dim3 grid(stream_blocks(lanes)), block(kBlock);
  const uintptr_t first = (uintptr_t)in + (size_t)head * (HALF ? 2 : 4);
  if ((first & 15u) == 0)
    hipLaunchKernelGGL((k_depthnet_unpack<HALF, 16>), grid, block, 0, s, in, depth, n, head, groups, mode);
  else if ((first & 3u) == 0)
    hipLaunchKernelGGL((k_depthnet_unpack<HALF, 4>), grid, block, 0, s, in, depth, n, head, groups, mode);
  else  // fp16 on an odd halfword; fp32 is always dword aligned, so this instantiation is the same kernel as the one above
    hipLaunchKernelGGL((k_depthnet_unpack<HALF, HALF ? 2 : 4>), grid, block, 0, s, in, depth, n, head, groups, mode);
}

}  // namespace
}  // namespace dms

using namespace dms;

extern "C" {

int dms_depthnet_pack(const void* rgb_dev, int rgb_channels, int width, int height, void* tensor_dev, int half, dms_stream st) {
  DMS_REQUIRE(rgb_dev && tensor_dev, "null argument");
  DMS_REQUIRE(rgb_channels == 3 || rgb_channels == 4, "rgb_channels must be 3 or 4");
  DMS_REQUIRE(width > 0 && height > 0 && (long long)width * height <= 0x7fffffffLL, "width and height must be positive, their product below 2^31");
  const int elem = half ? 2 : 4;
  DMS_REQUIRE(((uintptr_t)tensor_dev & (uintptr_t)(elem - 1)) == 0, "tensor_dev is not aligned to its element");
  const unsigned n = (unsigned)width * (unsigned)height;
  hipStream_t s = (hipStream_t)st;
  const unsigned char* rgb = reinterpret_cast<const unsigned char*>(rgb_dev);
  if (((size_t)n * elem) % 16 == 0) {  // the three planes share their alignment
    unsigned head, groups;
    split(tensor_dev, n, elem, half ? 8 : 4, &head, &groups);
    if (rgb_channels == 3) {
      if (half) launch_pack<3, true>(rgb, tensor_dev, n, head, groups, s);
      else launch_pack<3, false>(rgb, tensor_dev, n, head, groups, s);
    } else {
      if (half) launch_pack<4, true>(rgb, tensor_dev, n, head, groups, s);
      else launch_pack<4, false>(rgb, tensor_dev, n, head, groups, s);
    }
  } else {
    const dim3 grid(stream_blocks(n)), block(kBlock);
    if (half)
      hipLaunchKernelGGL(k_depthnet_pack_elementwise<true>, grid, block, 0, s, rgb, rgb_channels, tensor_dev, n);
    else
      hipLaunchKernelGGL(k_depthnet_pack_elementwise<false>, grid, block, 0, s, rgb, rgb_channels, tensor_dev, n);
  }
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int dms_depthnet_unpack(const void* tensor_dev, int half, int width, int height, unsigned short* depth_dev, int mode, dms_stream st) {
  DMS_REQUIRE(tensor_dev && depth_dev, "null argument");
  DMS_REQUIRE(width > 0 && height > 0 && (long long)width * height <= 0x7fffffffLL, "width and height must be positive, their product below 2^31");
  DMS_REQUIRE(mode == DMS_DEPTHNET_RUNTIME || mode == DMS_DEPTHNET_TRUNCATE, "unknown mode");
  DMS_REQUIRE(((uintptr_t)tensor_dev & (uintptr_t)(half ? 1 : 3)) == 0 && ((uintptr_t)depth_dev & 1u) == 0,
              "tensor_dev or depth_dev is not aligned to its element");
  const unsigned n = (unsigned)width * (unsigned)height;
  if (half)
    launch_unpack<true>(tensor_dev, depth_dev, n, mode, (hipStream_t)st);
  else
    launch_unpack<false>(tensor_dev, depth_dev, n, mode, (hipStream_t)st);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

}  // extern "C"
