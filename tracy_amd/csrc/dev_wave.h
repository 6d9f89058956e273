// dev_wave.h -- the 64-lane wave that the bodies (dp_kernels.h, band16.h, front.h, the *_wave.h headers) are written against, on the
// device.  A body is a template over its wave W and calls nothing of the machine but W's members; the same text runs on the fibers of
// tests/emu/host_wave.h.  The wave concept -- every member a body may call, what it must mean, and which wave provides it:
//
//   lane()                  0 .. 63, this lane's index in its wave                                                        every wave
//   ballot(p)               bit l = p of lane l, the same word in every lane                                              every wave
//   bcast(x, src_lane)      lane src_lane's x; src_lane may differ from lane to lane (DecompDevWave: it may not)          every wave
//   reduce(x, f)            f folded over the 64 x in some order, f associative and commutative; the same in every lane   every wave
//   sum / umin / umax(x)    reduce with +, unsigned min, unsigned max                                                     every wave
//   excl_sum(x)             the sum of x over the lanes below this one (lane 0: 0)                                        every wave
//   sync()                  LDS and global words written by lanes of this wave before it are seen by lanes of this wave
//                           behind it, and no lane passes before all have arrived   every wave but MsaDevWave (its bodies share nothing)
//   sync_global()           the same for global words alone, without the promise to arrive together    DeviceWave, DeviceWave16, SoloWave
//   lds()                   the wave's own LDS, 16-byte aligned, sized by the launch or the wave   DeviceWave, DeviceWave16, DecompDevWave, SoloWave
//   shift_up / shift_up_row / shift_up_or(x[, first])   lane L <- lane L - 1 of the wave / of its row of sixteen          DeviceWave
//   rot16(x), rot(x, integral_constant<16 | 4>)         lane j <- lane j - 1 of its row of sixteen / its quad, cyclic     DeviceWave16
// Every member but lane() and lds() is called by all 64 lanes together, with whatever arguments: never under divergence.
//
// DevWaveOps holds what is the same on every device wave; a wave that adds to it or overrides a member stays beside its kernels:
// DeviceWave (dp_kernels.hip), DeviceWave16 (band16.hip), DecompDevWave (decompose_kernels.hip), VarDevWave (variants.hip).  The
// members are not virtual: a wave that overrides reduce restates sum / umin / umax over its own.
#ifndef TRACY_AMD_DEV_WAVE_H
#define TRACY_AMD_DEV_WAVE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tracyhip {

// WAVE_IS_BLOCK: the workgroup is one wave of 64 threads; else several waves share it, each with its own work
template <bool WAVE_IS_BLOCK>
struct DevWaveOps {
  __device__ __forceinline__ uint32_t lane() const { return WAVE_IS_BLOCK ? threadIdx.x : threadIdx.x & 63u; }
  __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ __forceinline__ uint32_t bcast(uint32_t x, uint32_t src_lane) const { return (uint32_t)__shfl((int)x, (int)src_lane, 64); }
  template <class F>
  __device__ __forceinline__ uint32_t reduce(uint32_t x, F f) const {  // butterfly, six shuffles
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = f(x, (uint32_t)__shfl_xor((int)x, o, 64));
    return x;
  }
  __device__ __forceinline__ uint32_t sum(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a + b; }); }
  __device__ __forceinline__ uint32_t umin(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
  __device__ __forceinline__ uint32_t umax(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a > b ? a : b; }); }
  __device__ __forceinline__ uint32_t excl_sum(uint32_t x) const {  // Hillis-Steele, six shuffles
    uint32_t v = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)v, o, 64);
      if ((int)lane() >= o) v += y;
    }
    return v - x;
  }
};

// the wave of assemble_wave.h (msa_batch.hip, denovo.hip): one workgroup of 64 threads, lane and ballot alone
using MsaDevWave = DevWaveOps<true>;

// One wave per trace, WAVES traces per workgroup, LDS_BYTES of a static LDS array each (basecall.hip, pad.hip).  Waves never wait for
// each other: the wave's own LDS and global writes become visible to its own lanes -- no other wave shares them -- by a memory fence and
// a wave barrier, not a workgroup barrier.
template <uint32_t WAVES, uint32_t LDS_BYTES>
struct SoloWave : DevWaveOps<false> {
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void sync_global() const { sync(); }
  __device__ __forceinline__ char* lds() const {
    __shared__ __attribute__((aligned(16))) char solo_smem[WAVES * LDS_BYTES];
    return solo_smem + (threadIdx.x >> 6) * LDS_BYTES;
  }
};

}  // namespace tracyhip
#endif
