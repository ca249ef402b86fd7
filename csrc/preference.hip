// Sequence-level objectives (DPO) on top of the fused cross-entropy, for gfx950.
//
// ce_fwd leaves the per-row NLL in row 0 of its stats and G = softmax - onehot in the logits buffer. A per-sequence
// log-probability is a segment sum of that NLL (seq_logp_sum); its backward weights every row of a sequence by one
// value r_s, and a per-row weight commutes with both LM-head backward GEMMs (dh = diag(r) (G W), dW = G^T (diag(r) h)),
// so the weight goes onto the two [T, hidden] operands (scale_rows_by_seq, csrc/scale_rows.hip), never onto the
// [T, vocab] one. dpo_pair_fwd
// turns the 2P sequence log-probabilities of P (chosen, rejected) pairs into the per-pair loss, its gradient
// coefficient and the reward statistics in one launch.
//
// No atomics: every value has one writer and a fixed summation order, so results are run-to-run identical.
#include "common.h"

namespace sftamd {

// One wave per sequence: lane l adds rows cu[s] + l, + 64, ... in order, then the fixed xor butterfly of wave_sum.
// Only rows of [cu[s], cu[s + 1]) are read, clamped to [0, M].
__global__ __launch_bounds__(256) void seq_logp_sum_kernel(const float* __restrict__ nll, const int* __restrict__ cu,
                                                           float* __restrict__ logps, int n_seqs, int M) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seqs) return;
  const int lane = threadIdx.x & 63;
  const int a = min(max(cu[s], 0), M);
  const int b = min(max(cu[s + 1], a), M);
  float acc = 0.f;
  for (int t = a + lane; t < b; t += WAVE) acc += nll[t];
  acc = wave_sum(acc);
  if (lane == 0) logps[s] = 0.f - acc;
}

at::Tensor seq_logp_sum(const at::Tensor& nll, const at::Tensor& cu_seqlens, int64_t n_seqs) {
  SFT_CHECK_CUDA(nll);
  SFT_CHECK(nll.scalar_type() == at::kFloat && nll.dim() == 1 && nll.is_contiguous(), "seq_logp_sum: nll fp32 [M]");
  SFT_CHECK(cu_seqlens.is_cuda() && cu_seqlens.scalar_type() == at::kInt && cu_seqlens.dim() == 1 &&
                cu_seqlens.is_contiguous(), "seq_logp_sum: cu_seqlens int32 [S + 1] on the GPU");
  SFT_CHECK(n_seqs >= 0 && n_seqs + 1 <= cu_seqlens.numel(), "seq_logp_sum: n_seqs over the segments of cu_seqlens");
  SFT_CHECK(nll.numel() < (1L << 31), "seq_logp_sum: M over int32");
  auto out = at::empty({n_seqs}, nll.options());
  if (n_seqs == 0) return out;
  SFT_TRACE("pref.seq_logp");
  seq_logp_sum_kernel<<<(unsigned)((n_seqs + 3) / 4), 256, 0, cur_stream()>>>(
      nll.data_ptr<float>(), cu_seqlens.data_ptr<int>(), out.data_ptr<float>(), (int)n_seqs, (int)nll.numel());
  SFT_LAUNCH_CHECK();
  return out;
}

// Pair p = sequences (2p chosen, 2p + 1 rejected). stats [5, P]: loss, coef (d(inv_pairs sum loss) / d logp_chosen; the
// rejected sequence's is its negative), reward_chosen, reward_rejected, delta. softplus(-z) and the sigmoid are
// common.h's softplus_sigmoid_neg (shared with csrc/reward.hip): no overflow at any z.
__global__ __launch_bounds__(256) void dpo_pair_fwd_kernel(const float* __restrict__ lp, const float* __restrict__ rlp,
                                                           const float* __restrict__ inv_pairs,
                                                           float* __restrict__ stats, int P, float beta) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float pc = lp[2 * p], pr = lp[2 * p + 1], rc = rlp[2 * p], rr = rlp[2 * p + 1];
  const float delta = (pc - pr) - (rc - rr);
  const float z = beta * delta;
  float loss, sig;  // softplus(-z), sigmoid(-z)
  softplus_sigmoid_neg(z, loss, sig);
  stats[p] = loss;
  stats[P + p] = (-beta * sig) * inv_pairs[0];
  stats[2 * P + p] = beta * (pc - rc);
  stats[3 * P + p] = beta * (pr - rr);
  stats[4 * P + p] = delta;
}

at::Tensor dpo_pair_fwd(const at::Tensor& logps, const at::Tensor& ref_logps, const at::Tensor& inv_pairs, double beta) {
  SFT_CHECK_CUDA(logps);
  SFT_CHECK(logps.scalar_type() == at::kFloat && logps.dim() == 1 && logps.is_contiguous() && logps.numel() % 2 == 0,
            "dpo_pair_fwd: logps fp32 [2 P]");
  SFT_CHECK(ref_logps.is_cuda() && ref_logps.scalar_type() == at::kFloat && ref_logps.is_contiguous() &&
                ref_logps.dim() == 1 && ref_logps.numel() == logps.numel(), "dpo_pair_fwd: ref_logps fp32 [2 P] on the GPU");
  SFT_CHECK(inv_pairs.is_cuda() && inv_pairs.scalar_type() == at::kFloat && inv_pairs.numel() == 1,
            "dpo_pair_fwd: inv_pairs a fp32 GPU scalar");
  const long P = logps.numel() / 2;
  SFT_CHECK(P < (1L << 28), "dpo_pair_fwd: too many pairs");
  auto stats = at::empty({5, P}, logps.options());
  if (P == 0) return stats;
  SFT_TRACE("pref.dpo_pair");
  dpo_pair_fwd_kernel<<<(unsigned)((P + 255) / 256), 256, 0, cur_stream()>>>(
      logps.data_ptr<float>(), ref_logps.data_ptr<float>(), inv_pairs.data_ptr<float>(), stats.data_ptr<float>(), (int)P,
      (float)beta);
  SFT_LAUNCH_CHECK();
  return stats;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("seq_logp_sum", &seq_logp_sum);
  m.impl("dpo_pair_fwd", &dpo_pair_fwd);
}

}  // namespace sftamd
