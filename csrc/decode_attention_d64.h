// Host launchers of the MFMA decode-attention split kernels (csrc/decode_attention_d64.hip); decode_attention /
// decode_attention_batched in csrc/decode_attention.hip check the arguments, allocate the partials, dispatch here on
// the cache's head_dim and run the append and combine kernels they share with head_dim 128.
#pragma once

#include "common.h"

namespace sftamd {
namespace decode64 {

constexpr int D = 64;  // the one head_dim instantiated and bound (the kernel is a template on it)

// One sequence. q [nq * 64] bf16, kc / vc [smax, nkv, 64] bf16, len_p one int32 on the device (clamped to smax),
// part_o [nkv, splits, rep, 64] / part_ml [nkv, splits, rep, 2] fp32 with splits = ceil(smax / 256); sl2 = scale *
// log2(e). q, kc, vc 16-byte aligned.
void launch_split(const u16* q, const u16* kc, const u16* vc, const int* len_p, float* part_o, float* part_ml, int nq,
                  int nkv, int smax, float sl2, hipStream_t st);
// B sequences. qkv [B, (nq + 2 nkv) * 64], kc / vc [B, smax, nkv, 64], lens [B] int32 on the device, part_o
// [B, nkv, splits, rep, 64], part_ml [B, nkv, splits, rep, 2].
void launch_split_batched(const u16* qkv, const u16* kc, const u16* vc, const int* lens, float* part_o, float* part_ml,
                          int B, int nq, int nkv, int smax, float sl2, hipStream_t st);

// Shared-prefix step of B = n_groups * G rows at head_dim hd (64 or 128), csrc/decode_attention_d64.hip: row b attends
// over prefix[b / G, :plens[b / G]] (pk / pv [n_groups, pmax, nkv, hd], plens [n_groups] int32, clamped to [0, pmax])
// and over its own slab kc / vc [B, sown, nkv, hd], whose live length is own = lens[b] - plens[b / G]. The append
// stores the step's K/V at own row own - 1 (own outside (0, sown]: the row is skipped and attends over its prefix
// alone). part_o [B, nkv, splits_total, rep, hd] / part_ml [.., 2] with splits_total = ceil(pmax / 256) +
// ceil(sown / 256): the prefix kernel fills the first ceil(pmax / 256) slots of every row, the suffix kernel the rest.
void launch_prefix_step(int hd, const u16* qkv, u16* kc, u16* vc, const int* lens, const u16* pk, const u16* pv,
                        const int* plens, float* part_o, float* part_ml, int B, int G, int nq, int nkv, int sown,
                        int pmax, float sl2, hipStream_t st);

}  // namespace decode64
}  // namespace sftamd
