// Staging and tile-order primitives shared by the MFMA kernels (gemm_tn / gemm_dgrad / gemm_wgrad / gemm_4w /
// attention): LDS-DMA issue, LDS fragment reads, the LDS chunk swizzles, counted waits, tile order. Everything here is
// __forceinline__ (or constexpr) and carries no state: a helper belongs here once two kernel families need the SAME
// thing; whatever differs between families stays in its own file.
#pragma once

#include "common.h"

namespace sftamd {

// ------------------------------------------------------------------------------ waits
// s_waitcnt immediate of gfx9: vmcnt[3:0] expcnt[6:4] lgkmcnt[11:8] vmcnt[5:4]<<14 (expcnt left at its maximum)
constexpr unsigned waitcnt_imm(int vm, int lgkm) {
  return (unsigned)((vm & 15) | (7 << 4) | ((lgkm & 15) << 8) | ((vm >> 4) << 14));
}

// ------------------------------------------------------------------------------ LDS-DMA
// 16 bytes per lane from a flat global address; the DMA writes LDS lane-linearly (1 KB per wave instruction), so any
// swizzle is applied on the GLOBAL source address.
__device__ __forceinline__ void glds16(const u16* src, char* dst) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                   (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
}

// The same through a buffer descriptor: the tile's base in the (wave-uniform) descriptor, each lane's byte offset in a
// VGPR fixed for the whole loop, the piece / K-step offset in an SGPR — no per-piece 64-bit VALU address arithmetic
// (the global_load_lds form costs a v_lshl_add_u64 per piece), as hipBLASLt's MT256x256x64 loop does.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
// Unbounded range, 32-bit offsets: the HOST launchers check that no offset of a launch can reach 2^32 bytes
// (csrc/gemm_4w.hip check_tr_span / check_row_span, csrc/gemm_tn.hip launch6); the kernels themselves do not.
__device__ __forceinline__ rsrc_t tile_rsrc(const u16* p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, 0xFFFFFFFFu, 0x00020000);
}
__device__ __forceinline__ void bldsx4(rsrc_t r, char* dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// ------------------------------------------------------------------------------ LDS fragment reads
typedef __attribute__((address_space(3))) s16x4 lds_s4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// 8 bf16 of one image row: ds_read_b128
__device__ __forceinline__ bf16x8 lds_row(const char* base, int off) { return *(const bf16x8*)(base + off); }

// Transposed fragment: two ds_read_b64_tr_b16, the second PITCH bytes (16 image rows at the callers) after the first
template <int PITCH>
__device__ __forceinline__ bf16x8 lds_tr(const char* base, int off) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + off));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + off + PITCH));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ------------------------------------------------------------------------------ LDS chunk swizzles
// ds_read_b128 is serviced in four NON-contiguous 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...). A
// fragment read has lane (g = lane >> 4, ii = lane & 15) at image row R + ii, 16-byte chunk g.
//
// The chunk selector S = {0, 2, 3, 1}: with 64-byte image rows the lane's slot in the 256-byte bank row is
// 4 (ii & 3) + (g ^ S(ii >> 2)), and S makes the 16 slots of every lane group distinct (the plain S(q) = q is 2-way).
__device__ __forceinline__ int swz_sel(int q) { return (0x78 >> (2 * q)) & 3; }

// 64-byte rows (32 bf16 of k; gemm_tn BK = 32, gemm_dgrad's dY image, gemm_4w's ROW operand)
__device__ __forceinline__ int swz64(int row, int ch) { return ch ^ swz_sel((row >> 2) & 3); }
// 128-byte rows (64 bf16 of k; the BK = 64 variants of gemm_tn and gemm_dgrad)
__device__ __forceinline__ int swz128(int row, int ch) { return ch ^ ((row >> 1) & 7); }

// 256-byte rows (128 bf16 = one whole bank row): TWO swizzles are in use, and they DIFFER in the low two bits:
//   swz256_q  ch ^ ((row & 3) << 2 | (row >> 2) & 3)     gemm_wgrad (both images), gemm_dgrad (the weight image)
//   swz256_s  ch ^ ((row & 3) << 2 | S((row >> 2) & 3))  attention (every [rows][128] image)
// swz256_s is conflict-free for the 16-byte row reads AND for the transposed ds_read_b64_tr_b16 reads (2 x 32 lanes),
// checked exhaustively against the MI355X lane groups (tools/lds_swizzle_check.py); swz256_q, which attention used
// before, was 2-way on both there. The GEMMs only do transposed reads of these images and have not been measured
// under swz256_s: moving them is a performance change of its own.
__device__ __forceinline__ int swz256_q(int row, int ch) { return ch ^ (((row & 3) << 2) | ((row >> 2) & 3)); }
__device__ __forceinline__ int swz256_s(int row, int ch) { return ch ^ (((row & 3) << 2) | swz_sel((row >> 2) & 3)); }

// ------------------------------------------------------------------------------ ring slots
// Slot i of up to six stage pointers kept as separate __restrict__ values (i is a compile-time constant after
// unrolling); a five-slot ring leaves b5 out.
__device__ __forceinline__ char* pick(int i, char* b0, char* b1, char* b2, char* b3, char* b4, char* b5 = nullptr) {
  switch (i) {
    case 0: return b0;
    case 1: return b1;
    case 2: return b2;
    case 3: return b3;
    case 4: return b4;
    default: return b5;
  }
}

// ------------------------------------------------------------------------------ tile order
constexpr int kTileGroup = 8;  // GROUP tile order: 8 blocks of the grouped axis share each panel of the other operand

// XCD-aware bijective remap of workgroup `orig` of `n`: workgroups are dealt round-robin to the 8 XCDs, so consecutive
// remapped ids land on ONE XCD and share its L2.
__device__ __forceinline__ int xcd_remap(int orig, int n) {
  const int xcd = orig & 7, q8 = n >> 3, r8 = n & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
}

// GROUP-blocked order over a grid of nbm x nbn tiles of BM x BN: `group` m-blocks at a time, m fastest within a group;
// (m0, n0) = the origin of tile `tile`.
template <int BM = 256, int BN = 256>
__device__ __forceinline__ void tile_origin(int tile, int nbm, int nbn, int group, int& m0, int& n0) {
  const int per_group = group * nbn;
  const int grp = tile / per_group, first = grp * group;
  const int gsz = min(nbm - first, group);
  const int in = tile - grp * per_group;
  m0 = (first + in % gsz) * BM;
  n0 = (in / gsz) * BN;
}

}  // namespace sftamd
