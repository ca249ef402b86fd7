// Row-wise ops on the packed qkv GEMM output (rope_ in elementwise.hip, qk_norm.hip, qkv_bias.hip): the lane layout of
// a head row, the rotate-half arithmetic, the column-sum tail of the backward kernels and the host argument checks.
//
// Lane layout (head_dim 128; qk_norm / qkv_bias): a head row is 128 bf16 = 256 bytes. Lane l of a wave owns row
// (l >> 3) of the wave's 8 rows and, with p = (l & 7) * 8, the elements p..p+7 and 64+p..64+p+7 of it: two 16-byte
// accesses, and every rotate-half pair (x[i], x[i + 64]) sits in ONE lane. A row reduction is three xor-shuffle steps
// (1, 2, 4) inside the 8-lane group; lanes l, l ^ 8, l ^ 16, l ^ 32 hold the same 16 columns of the wave's 8 rows. A
// block is 4 waves = 32 rows per step.
#pragma once

#include "common.h"

namespace sftamd {

// sum over the 8 lanes of a head row
__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// 8 consecutive fp32 (a lane's slice of a cos / sin row): two 16-byte loads
__device__ __forceinline__ void load8f(const float* p, float* f) {
  *(float4*)&f[0] = ((const float4*)p)[0];
  *(float4*)&f[4] = ((const float4*)p)[1];
}

// rotate_half of one pair (t1, t2) = (x[i], x[i + D/2]): (t1 c - t2 s, t2 c + t1 s). The operation order is part of
// the contract (kernels that promise bitwise-equal results share it).
__device__ __forceinline__ void rotate_pair_fwd(float t1, float t2, float c, float s, float& o1, float& o2) {
  o1 = t1 * c - t2 * s;
  o2 = t2 * c + t1 * s;
}
// ... of a lane's 8 pairs; the outputs may be the inputs
__device__ __forceinline__ void rotate_half_fwd(const float* x1, const float* x2, const float* c, const float* s,
                                                float* o1, float* o2) {
#pragma unroll
  for (int i = 0; i < 8; ++i) rotate_pair_fwd(x1[i], x2[i], c[i], s[i], o1[i], o2[i]);
}
// the inverse (= the transpose: the backward): (d1 c + d2 s, d2 c - d1 s)
__device__ __forceinline__ void rotate_pair_inv(float d1, float d2, float c, float s, float& o1, float& o2) {
  o1 = d1 * c + d2 * s;
  o2 = d2 * c - d1 * s;
}
__device__ __forceinline__ void rotate_half_inv(const float* d1, const float* d2, const float* c, const float* s,
                                                float* o1, float* o2) {
#pragma unroll
  for (int i = 0; i < 8; ++i) rotate_pair_inv(d1[i], d2[i], c[i], s[i], o1[i], o2[i]);
}

// Column sums of a wave: acc = the lane's 16 columns (p..p+7, 64+p..64+p+7) summed over its rows -> red[128], the
// wave's sums over its 8 row groups (shuffles over lanes 8 / 16 / 32, fixed order). Every lane of the wave must be here.
__device__ __forceinline__ void wave_colsum128(float (&acc)[16], float* red, int lane, int p) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) acc[i] += __shfl_xor(acc[i], o, 64);
  }
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[p + i] = acc[i];
      red[64 + p + i] = acc[8 + i];
    }
  }
}

// Host checks of "packed bf16 qkv [.., ld] + fp32 cos / sin [M, head_dim / 2]" for the kernels' 16-byte accesses;
// returns M. The row must hold the n_q + n_kv rotated heads (whole_row: be exactly the n_q + 2 n_kv heads).
inline long check_qkv_rows(const char* op, const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                           int64_t n_q, int64_t n_kv, int64_t head_dim, bool whole_row) {
  SFT_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous() && qkv.dim() >= 1, op,
            ": qkv must be a contiguous bfloat16 GPU tensor");
  SFT_CHECK(head_dim > 0 && head_dim % 16 == 0, op, ": head_dim must be a multiple of 16");
  SFT_CHECK(n_q >= 0 && n_kv >= 0, op, ": head counts");
  const long ld = qkv.size(-1);
  SFT_CHECK(whole_row ? ld == (n_q + 2 * n_kv) * head_dim : (ld >= (n_q + n_kv) * head_dim && ld % 8 == 0), op,
            ": qkv row width");
  SFT_CHECK(cos.is_cuda() && sin.is_cuda() && cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat, op,
            ": cos/sin must be fp32 GPU tensors");
  SFT_CHECK(cos.is_contiguous() && sin.is_contiguous(), op, ": cos/sin contiguous");
  const long M = ld ? qkv.numel() / ld : 0;
  SFT_CHECK(cos.numel() == M * (head_dim / 2) && sin.numel() == cos.numel(), op, ": cos table shape");
  auto al16 = [](const at::Tensor& t) { return ((uintptr_t)t.data_ptr() & 15) == 0; };
  SFT_CHECK(al16(qkv) && al16(cos) && al16(sin), op, ": 16-byte aligned tensors");
  return M;
}

// elementwise.hip: rotate the q and k heads of qkv in place (inverse: by -angle)
void rope_(at::Tensor qkv, const at::Tensor& cos, const at::Tensor& sin, int64_t n_q, int64_t n_kv, int64_t head_dim,
           bool inverse);

}  // namespace sftamd
