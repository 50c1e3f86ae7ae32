// The CDNA4 (gfx950) device primitives of the library, each defined ONCE: vector types, MFMA
// wrappers, LDS-DMA, transposed LDS reads and the zero block.  Included by scl_common.h, so every
// translation unit sees them.  Helpers that belong to one kernel (nv_glds16s in netvlad.hip) stay
// with that kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // 8 packed bf16: one MFMA operand
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));      // what a transposed LDS read returns

// ---- MFMA ------------------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32], exact f32 (a k-ordered
// fmaf chain).  Lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].
// Accumulator register r of lane l is D[row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][col = l & 31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int acc_row(int reg, int half) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * half;
}
// v_mfma_f32_16x16x4_f32: lane (i = l & 15, g = l >> 4) supplies A[i][k = g] and B[k = g][j = i];
// accumulator register r is D[row = 4 g + r][col = i]
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// v_mfma_f32_32x32x16_bf16 and v_mfma_f32_16x16x32_bf16: a lane's operand is 8 consecutive bf16 of
// the contraction index (16 bytes, k = 8 (l >> 5) + e resp. 8 (l >> 4) + e); accumulators as above
__device__ __forceinline__ f32x16 mfma32b(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16b(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- LDS-DMA ---------------------------------------------------------------------------
// global_load_lds_dwordx4: one wave instruction copies 64 x 16 bytes from global memory into 1 KB
// of CONSECUTIVE LDS at the wave-uniform byte address `lds_byte` (lane l lands at lds_byte + 16 l)
// — no staging registers, no ds_write pass, many more bytes in flight per CU.  The LDS image is
// lane-linear; a swizzle goes on the SOURCE address.
//   * Issued as inline asm so that hipcc does not order it against the LDS reads of the OTHER
//     buffer (with the builtin it waits vmcnt(0) before the next ds_read: no overlap at all).  The
//     block saves m0, points it at the destination and restores it.
//   * Nobody waits for it but the calling kernel: s_waitcnt vmcnt(n) before the barrier that
//     hands the buffer over.
//   * Lanes whose source lies outside the image must still read something: the global forms point
//     them at zero_block, the buffer form lets the hardware's bounds check return zeros.
static __device__ uint4 zero_block[4];               // never written: zeros

__device__ __forceinline__ unsigned lds_byte_of(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
// per-lane 64-bit source address
__device__ __forceinline__ void glds16(const void* src, unsigned lds_byte) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds_byte)
      : "memory");
}
// wave-uniform base pointer (an SGPR pair) and a 32-bit byte offset per lane: no vector
// instruction for the address at all
__device__ __forceinline__ void glds16_s(const void* base, unsigned off_bytes, unsigned lds_byte) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(off_bytes), "s"(base), "s"(lds_byte)
      : "memory");
}
// through a BUFFER RESOURCE (buffer_load_dwordx4 ... offen lds): the same 1-KB copy, with the
// hardware's bounds check on every lane's byte offset — an offset at or beyond num_records, or a
// negative one (it wraps to > 2^31), delivers ZEROS (scripts/buffer_lds_probe.hip).  With one
// resource per image the rows of a halo window that lie above or below the image need no per-lane
// test, no zero block and no select: one v_add per chunk instead of ~11 vector instructions.
// rsrc: {base lo, base hi (stride 0), num_records in bytes, 0x00020000}, wave-uniform.
__device__ __forceinline__ void blds16(u32x4 rsrc, unsigned voff_bytes, unsigned lds_byte) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff_bytes), "s"(rsrc), "s"(lds_byte)
      : "memory");
}
__device__ __forceinline__ u32x4 image_rsrc(const unsigned short* base, int64_t first_elem, unsigned bytes) {
  const unsigned long long a = (unsigned long long)(base + first_elem);
  return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a),
               (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu)),
               (unsigned)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}

// ---- transposed LDS reads --------------------------------------------------------------
// ds_read_b64_tr_b16: the 16 lanes of a group address four rows of 16 bf16 (lane 4 q + p: row q,
// columns 4 p .. + 3); lane i receives column i of the four rows.  lds_tr16 reads at a pointer into
// LDS and returns the register pair as the builtin delivers it (the caller bit-casts: a uint2
// returned from here reaches the register allocator in another order), lds_tr16_at reads at an LDS
// byte address; tr_pair is two reads `step4` elements (four rows) apart: 8 consecutive rows of one
// column, the 16 bytes of a bf16 MFMA operand.
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ s16x4 lds_tr16(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
__device__ __forceinline__ uint2 lds_tr16_at(unsigned byte) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)byte);
  return __builtin_bit_cast(uint2, v);
}
__device__ __forceinline__ u32x4 tr_pair(const unsigned short* a0, int step4) {
  const uint2 l2 = __builtin_bit_cast(uint2, lds_tr16(a0));
  const uint2 h2 = __builtin_bit_cast(uint2, lds_tr16(a0 + step4));
  return u32x4{l2.x, l2.y, h2.x, h2.y};
}
