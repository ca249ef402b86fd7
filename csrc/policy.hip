// Per-token policy objectives (GRPO) on top of the fused cross-entropy, for gfx950.
//
// ce_fwd at the sampling temperature tau leaves the per-row NLL of softmax(x / tau) in row 0 of its stats and
// G = softmax(x / tau) - onehot in the logits buffer. grpo_token_fwd turns that NLL (lp = -nll), the sampler's / an
// earlier pass's log-probabilities and the reference's into the clipped-ratio loss with TRL's k3 KL estimator, per
// completion row, plus its derivative c = dl / dlp. As in csrc/preference.hip a row weight commutes with both LM-head
// backward GEMMs (dh = diag(c) (G W), dW = G^T (diag(c) h)), so c goes onto the two [T, hidden] operands (scale_rows, csrc/scale_rows.hip),
// never onto the [T, vocab] one.
//
// No atomics: every value has one writer and a fixed summation order, so results are run-to-run identical.
#include "common.h"

namespace sftamd {

// One wave per sequence s (rows [cu[s], cu[s + 1]) clamped to [0, M]); a completion row has labels[t] >= 0. Pass 1
// counts the sequence's completion rows (the per-sequence mean's divisor), pass 2 writes the rows and keeps the sums;
// lane l visits rows cu[s] + l, + 64, ... in order, then the fixed xor butterfly of wave_sum. ``rows`` arrives zeroed:
// rows outside every sequence keep their +0, rows inside are all written here. The twin is ref.grpo_token
// (ops/reference.py), with the same expressions in the same order.
//   r = exp(lp - old) (1 without old), lo = 1 - eps_low, hi = 1 + eps_high
//   l = -min(r A, clamp(r, lo, hi) A) + beta (exp(d) - d - 1), d = ref - lp (no KL term without ref)
//   c = -A r [r A <= clamp(r) A] + beta (1 - exp(d))                 (both through em = expm1(d): em - d, -em)
//   rows[0][t] = w l, rows[1][t] = w c, w = inv_norm (/ max(completion rows, 1) with per_seq_mean)
//   seq[.][s] = sum of (w l, 1, [r < lo and A < 0], [r > hi and A > 0], exp(d) - d - 1, r) over the completion rows
__global__ __launch_bounds__(256) void grpo_token_fwd_kernel(
    const float* __restrict__ nll, const float* __restrict__ old_lp, const float* __restrict__ ref_lp,
    const int64_t* __restrict__ labels, const float* __restrict__ adv, const int* __restrict__ cu,
    const float* __restrict__ inv_norm, float* __restrict__ rows, float* __restrict__ seq, int n_seqs, int M,
    float eps_low, float eps_high, float beta, int per_seq_mean) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seqs) return;
  const int lane = threadIdx.x & 63;
  const int a = min(max(cu[s], 0), M);
  const int b = min(max(cu[s + 1], a), M);
  float cnt = 0.f;
  for (int t = a + lane; t < b; t += WAVE) cnt += labels[t] >= 0 ? 1.f : 0.f;
  cnt = wave_sum(cnt);  // (exact: whole numbers below 2^24)
  float w = inv_norm[0];
  if (per_seq_mean) w = w / fmaxf(cnt, 1.f);
  const float A = adv[s];
  const float lo = 1.f - eps_low, hi = 1.f + eps_high;
  float sl = 0.f, slow = 0.f, shigh = 0.f, skl = 0.f, sr = 0.f;
  for (int t = a + lane; t < b; t += WAVE) {
    float l = 0.f, c = 0.f;
    if (labels[t] >= 0) {
      const float lp = 0.f - nll[t];
      const float r = old_lp ? expf(lp - old_lp[t]) : 1.f;
      const float t1 = r * A;
      const float t2 = fminf(fmaxf(r, lo), hi) * A;
      l = 0.f - fminf(t1, t2);
      c = t1 <= t2 ? 0.f - t1 : 0.f;
      if (ref_lp) {
        const float d = ref_lp[t] - lp;
        const float em = expm1f(d);  // exp(d) - 1 without the cancellation at small d
        const float kl = em - d;
        l = l + beta * kl;
        c = c - beta * em;
        skl += kl;
      }
      l = w * l;
      c = w * c;
      sl += l;
      slow += (r < lo && A < 0.f) ? 1.f : 0.f;
      shigh += (r > hi && A > 0.f) ? 1.f : 0.f;
      sr += r;
    }
    rows[t] = l;
    rows[(long)M + t] = c;
  }
  sl = wave_sum(sl);
  slow = wave_sum(slow);
  shigh = wave_sum(shigh);
  skl = wave_sum(skl);
  sr = wave_sum(sr);
  if (lane == 0) {
    const long S = n_seqs;
    seq[s] = sl;
    seq[S + s] = cnt;
    seq[2 * S + s] = slow;
    seq[3 * S + s] = shigh;
    seq[4 * S + s] = skl;
    seq[5 * S + s] = sr;
  }
}

std::tuple<at::Tensor, at::Tensor> grpo_token_fwd(const at::Tensor& nll, const c10::optional<at::Tensor>& old_logps,
                                                  const c10::optional<at::Tensor>& ref_logps, const at::Tensor& labels,
                                                  const at::Tensor& adv, const at::Tensor& cu_seqlens, int64_t n_seqs,
                                                  const at::Tensor& inv_norm, double eps_low, double eps_high,
                                                  double beta, bool per_seq_mean) {
  SFT_CHECK_CUDA(nll);
  SFT_CHECK(nll.scalar_type() == at::kFloat && nll.dim() == 1 && nll.is_contiguous(), "grpo_token_fwd: nll fp32 [M]");
  const long M = nll.numel();
  SFT_CHECK(M < (1L << 31), "grpo_token_fwd: M over int32");
  auto row_vec = [&](const c10::optional<at::Tensor>& t) {
    return !t.has_value() || (t->is_cuda() && t->scalar_type() == at::kFloat && t->dim() == 1 && t->is_contiguous() &&
                              t->numel() == M);
  };
  SFT_CHECK(row_vec(old_logps), "grpo_token_fwd: old_logps fp32 [M] on the GPU");
  SFT_CHECK(row_vec(ref_logps), "grpo_token_fwd: ref_logps fp32 [M] on the GPU");
  SFT_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.is_contiguous() && labels.numel() == M,
            "grpo_token_fwd: labels int64 [M] on the GPU");
  SFT_CHECK(cu_seqlens.is_cuda() && cu_seqlens.scalar_type() == at::kInt && cu_seqlens.dim() == 1 &&
                cu_seqlens.is_contiguous(), "grpo_token_fwd: cu_seqlens int32 [S + 1] on the GPU");
  SFT_CHECK(n_seqs >= 0 && n_seqs + 1 <= cu_seqlens.numel(), "grpo_token_fwd: n_seqs over the segments of cu_seqlens");
  SFT_CHECK(adv.is_cuda() && adv.scalar_type() == at::kFloat && adv.is_contiguous() && adv.numel() == n_seqs,
            "grpo_token_fwd: adv fp32 [n_seqs] on the GPU");
  SFT_CHECK(inv_norm.is_cuda() && inv_norm.scalar_type() == at::kFloat && inv_norm.numel() == 1,
            "grpo_token_fwd: inv_norm a fp32 GPU scalar");
  SFT_CHECK(eps_low >= 0.0 && eps_low < 1.0 && eps_high >= 0.0, "grpo_token_fwd: eps_low in [0, 1), eps_high >= 0");
  SFT_CHECK(beta >= 0.0, "grpo_token_fwd: beta must be >= 0");
  auto rows = at::zeros({2, M}, nll.options());
  auto seq = at::empty({6, n_seqs}, nll.options());
  if (n_seqs == 0 || M == 0) return {rows, seq.zero_()};
  SFT_TRACE("policy.grpo_token");
  grpo_token_fwd_kernel<<<(unsigned)((n_seqs + 3) / 4), 256, 0, cur_stream()>>>(
      nll.data_ptr<float>(), old_logps.has_value() ? old_logps->data_ptr<float>() : nullptr,
      ref_logps.has_value() ? ref_logps->data_ptr<float>() : nullptr, labels.data_ptr<int64_t>(), adv.data_ptr<float>(),
      cu_seqlens.data_ptr<int>(), inv_norm.data_ptr<float>(), rows.data_ptr<float>(), seq.data_ptr<float>(), (int)n_seqs,
      (int)M, (float)eps_low, (float)eps_high, (float)beta, per_seq_mean ? 1 : 0);
  SFT_LAUNCH_CHECK();
  return {rows, seq};
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("grpo_token_fwd", &grpo_token_fwd);
}

}  // namespace sftamd
