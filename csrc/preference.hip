// Sequence-level objectives (DPO) on top of the fused cross-entropy, for gfx950.
//
// ce_fwd leaves the per-row NLL in row 0 of its stats and G = softmax - onehot in the logits buffer. A per-sequence
// log-probability is a segment sum of that NLL (seq_logp_sum); its backward weights every row of a sequence by one
// value r_s, and a per-row weight commutes with both LM-head backward GEMMs (dh = diag(r) (G W), dW = G^T (diag(r) h)),
// so the weight goes onto the two [T, hidden] operands (scale_rows_by_seq), never onto the [T, vocab] one. dpo_pair_fwd
// turns the 2P sequence log-probabilities of P (chosen, rejected) pairs into the per-pair loss, its gradient
// coefficient and the reward statistics in one launch.
//
// No atomics: every value has one writer and a fixed summation order, so results are run-to-run identical.
#include "common.h"

#include <algorithm>

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

// out[t, :] = bf16(float(x[t, :]) * (coef[s(t)] * gscale)), s(t) the segment of row t; rows at or past cu[n_seqs]: +0.
// blockIdx.y strides the rows, so the row and its segment search (over cu[1 .. n_seqs]) are uniform in the block: once
// per row, scalar loads. x and out may be the same buffer (the in-place form): every vector is read before it is
// written, by the thread that writes it.
__global__ __launch_bounds__(256) void scale_rows_by_seq_kernel(const u16* x, u16* out, const float* __restrict__ coef,
                                                                const int* __restrict__ cu,
                                                                const float* __restrict__ gscale, long M, int H,
                                                                int n_seqs) {
  const int k = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (k >= H) return;
  const float g = gscale[0];
  for (long t = blockIdx.y; t < M; t += gridDim.y) {
    int lo = 0, hi = n_seqs;  // lo = number of boundaries cu[1 .. n_seqs] at or below t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long)cu[mid + 1] <= t) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= n_seqs) {
      *(uint4*)(out + t * H + k) = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    const float c = coef[lo] * g;
    float v[8];
    unpack8(*(const uint4*)(x + t * H + k), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] *= c;
    *(uint4*)(out + t * H + k) = pack8(v);
  }
}

static void scale_rows_launch(const at::Tensor& x, at::Tensor& out, const at::Tensor& coef, const at::Tensor& cu,
                              int64_t n_seqs, const at::Tensor& gscale) {
  SFT_CHECK_CUDA(x);
  SFT_CHECK_BF16(x);
  SFT_CHECK_CONTIG(x);
  SFT_CHECK(x.dim() == 2 && x.size(1) % 8 == 0, "scale_rows_by_seq: x [M, H], H a multiple of 8");
  SFT_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat && coef.is_contiguous() && coef.numel() == n_seqs,
            "scale_rows_by_seq: coef fp32 [n_seqs] on the GPU");
  SFT_CHECK(cu.is_cuda() && cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.is_contiguous(),
            "scale_rows_by_seq: cu_seqlens int32 [S + 1] on the GPU");
  SFT_CHECK(n_seqs >= 0 && n_seqs + 1 <= cu.numel(), "scale_rows_by_seq: n_seqs over the segments of cu_seqlens");
  SFT_CHECK(gscale.is_cuda() && gscale.scalar_type() == at::kFloat && gscale.numel() == 1,
            "scale_rows_by_seq: gscale a fp32 GPU scalar");
  const long M = x.size(0);
  const int H = x.size(1);
  if (M == 0 || H == 0) return;
  dim3 grid((H / 8 + 255) / 256, (unsigned)std::min<long>(M, 65535));
  SFT_TRACE("pref.scale_rows");
  scale_rows_by_seq_kernel<<<grid, 256, 0, cur_stream()>>>((const u16*)x.data_ptr(), (u16*)out.data_ptr(),
                                                           coef.data_ptr<float>(), cu.data_ptr<int>(),
                                                           gscale.data_ptr<float>(), M, H, (int)n_seqs);
  SFT_LAUNCH_CHECK();
}

at::Tensor scale_rows_by_seq(const at::Tensor& x, const at::Tensor& coef, const at::Tensor& cu_seqlens, int64_t n_seqs,
                             const at::Tensor& gscale) {
  SFT_CHECK_CUDA(x);
  auto out = at::empty_like(x);
  scale_rows_launch(x, out, coef, cu_seqlens, n_seqs, gscale);
  return out;
}

void scale_rows_by_seq_(at::Tensor x, const at::Tensor& coef, const at::Tensor& cu_seqlens, int64_t n_seqs,
                        const at::Tensor& gscale) {
  scale_rows_launch(x, x, coef, cu_seqlens, n_seqs, gscale);
}

// Pair p = sequences (2p chosen, 2p + 1 rejected). stats [5, P]: loss, coef (d(inv_pairs sum loss) / d logp_chosen; the
// rejected sequence's is its negative), reward_chosen, reward_rejected, delta. softplus(-z) as max(-z, 0) +
// log1p(exp(-|z|)) and the sigmoid through exp(-|z|) only: no overflow at any z.
__global__ __launch_bounds__(256) void dpo_pair_fwd_kernel(const float* __restrict__ lp, const float* __restrict__ rlp,
                                                           const float* __restrict__ inv_pairs,
                                                           float* __restrict__ stats, int P, float beta) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float pc = lp[2 * p], pr = lp[2 * p + 1], rc = rlp[2 * p], rr = rlp[2 * p + 1];
  const float delta = (pc - pr) - (rc - rr);
  const float z = beta * delta;
  const float e = expf(-fabsf(z));
  const float loss = fmaxf(-z, 0.f) + log1pf(e);
  const float sig = (z >= 0.f ? e : 1.f) / (1.f + e);  // sigmoid(-z)
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
  m.impl("scale_rows_by_seq", &scale_rows_by_seq);
  m.impl("scale_rows_by_seq_", &scale_rows_by_seq_);
  m.impl("dpo_pair_fwd", &dpo_pair_fwd);
}

}  // namespace sftamd
