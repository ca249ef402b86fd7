// Host launchers of the head_dim-64 flash-attention kernels (csrc/attention_d64.hip); flash_fwd / flash_bwd /
// flash_bwd_rope in csrc/attention.hip check the arguments, allocate the tensors and dispatch here on head_dim.
#pragma once

#include "common.h"

namespace sftamd {
namespace attn64 {

constexpr int D = 64;  // head_dim (Llama-3.2-1B, SmolLM2)

// out [total, nq * 64] bf16, lse [nq, total] fp32 (natural log); sl2 = scale * log2(e)
void launch_fwd(const u16* qkv, u16* out, float* lse, const int* cu, int nq, int nkv, int total, int nseq,
                int max_seqlen, float sl2, int causal, hipStream_t st);
// delta[h][m] = sum_d dO[m, h, d] * O[m, h, d]
void launch_delta(const u16* dout, const u16* out, float* delta, int total, int nq, hipStream_t st);
// dqkv in the packed layout: the GQA-grouped dK / dV kernel, then the dQ kernel (both recompute S and dP)
void launch_bwd(const u16* qkv, const u16* dout, const float* lse, const float* delta, const int* cu, u16* dqkv, int nq,
                int nkv, int total, int nseq, int max_seqlen, float sl2, float scale, int causal, hipStream_t st);

}  // namespace attn64
}  // namespace sftamd
