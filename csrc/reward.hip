// Reward modelling on the trunk's hidden states, for gfx950: the score head and the pairwise (Bradley-Terry) loss.
//
// A reward model's score is the dot product of the LAST row of each sequence with one weight vector, so neither a
// [T, vocab] GEMM nor a [T, 1] one runs: seq_score_fwd reads one row per sequence, seq_score_bwd writes one row per
// sequence of dh (every other row is +0) and sums the same rows into dw. reward_pair_fwd turns the 2P scores of P
// (chosen, rejected) pairs into the per-pair loss, both gradient coefficients and the margin in one launch.
//
// Segment s of cu_seqlens is [a, b) with a = clamp(cu[s], 0, M), b = clamp(cu[s + 1], a, M) (seq_logp_sum's clamping);
// its last row is b - 1, an empty segment has none. cu_seqlens must be non-decreasing, as the attention kernels
// require: then no two segments share a last row and every row of dh has one writer.
//
// No atomics: every value has one writer and a fixed summation order, so results are run-to-run identical. The twins
// (ops/reference.py seq_score, seq_score_bwd, reward_pair) repeat the expressions and their order; contraction is off
// so that dh and dw are bit-equal to them.
#include "common.h"

namespace sftamd {

// One wave per sequence, four per block. Lane l takes the 16-byte chunks l, l + 64, ... of the row and adds its
// products in element order into one fp32 accumulator; then the fixed xor butterfly of wave_sum.
__global__ __launch_bounds__(256) void seq_score_fwd_kernel(const u16* __restrict__ h, const u16* __restrict__ w,
                                                            const int* __restrict__ cu, float* __restrict__ scores,
                                                            int n_seqs, int M, int H) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seqs) return;
  const int lane = threadIdx.x & 63;
  const int a = min(max(cu[s], 0), M);
  const int b = min(max(cu[s + 1], a), M);
  if (b <= a) {
    if (lane == 0) scores[s] = 0.f;
    return;
  }
  const uint4* row = reinterpret_cast<const uint4*>(h + (long)(b - 1) * H);
  const uint4* wv = reinterpret_cast<const uint4*>(w);
  float acc = 0.f;
  for (int c = lane; c < H / 8; c += WAVE) {
    float hf[8], wf[8];
    unpack8(row[c], hf);
    unpack8(wv[c], wf);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += hf[i] * wf[i];
  }
  acc = wave_sum(acc);
  if (lane == 0) scores[s] = acc;
}

// dh's one non-zero row per non-empty segment: row b - 1 = bf16(g_s * float(w_j)), one fp32 product and one rounding.
// One wave per sequence, the chunks split as in the forward. dh arrives zeroed.
__global__ __launch_bounds__(256) void seq_score_dh_kernel(const float* __restrict__ g, const u16* __restrict__ w,
                                                           const int* __restrict__ cu, u16* __restrict__ dh, int n_seqs,
                                                           int M, int H) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seqs) return;
  const int lane = threadIdx.x & 63;
  const int a = min(max(cu[s], 0), M);
  const int b = min(max(cu[s + 1], a), M);
  if (b <= a) return;  // (cu[s + 1] - 1 would name the previous segment's last row)
  const float gs = g[s];
  uint4* row = reinterpret_cast<uint4*>(dh + (long)(b - 1) * H);
  const uint4* wv = reinterpret_cast<const uint4*>(w);
  for (int c = lane; c < H / 8; c += WAVE) {
    float wf[8];
    unpack8(wv[c], wf);
#pragma unroll
    for (int i = 0; i < 8; ++i) wf[i] = gs * wf[i];
    row[c] = pack8(wf);
  }
}

// dw[j] = sum over the non-empty segments, in increasing s, of g_s * float(h[last_s, j]). One thread owns a 16-byte
// column group and walks the sequences (the segment bounds are wave-uniform loads).
__global__ __launch_bounds__(256) void seq_score_dw_kernel(const float* __restrict__ g, const u16* __restrict__ h,
                                                           const int* __restrict__ cu, float* __restrict__ dw, int n_seqs,
                                                           int M, int H) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= H / 8) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n_seqs; ++s) {
    const int a = min(max(cu[s], 0), M);
    const int b = min(max(cu[s + 1], a), M);
    if (b <= a) continue;
    const float gs = g[s];
    float hf[8];
    unpack8(reinterpret_cast<const uint4*>(h + (long)(b - 1) * H)[c], hf);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += gs * hf[i];
  }
  float4* out = reinterpret_cast<float4*>(dw + (long)c * 8);
  out[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  out[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

static void check_score_args(const char* op, const at::Tensor& h, const at::Tensor& w, const at::Tensor& cu_seqlens,
                             int64_t n_seqs) {
  SFT_CHECK(h.is_cuda() && h.scalar_type() == at::kBFloat16 && h.dim() == 2 && h.is_contiguous(), op,
            ": h bf16 [M, H], contiguous, on the GPU");
  SFT_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.dim() == 1 && w.is_contiguous() &&
                w.numel() == h.size(1), op, ": w bf16 [H] on the GPU");
  SFT_CHECK(h.get_device() == w.get_device() && h.get_device() == cu_seqlens.get_device(), op,
            ": h, w and cu_seqlens on one device");
  SFT_CHECK(cu_seqlens.is_cuda() && cu_seqlens.scalar_type() == at::kInt && cu_seqlens.dim() == 1 &&
                cu_seqlens.is_contiguous(), op, ": cu_seqlens int32 [S + 1] on the GPU");
  SFT_CHECK(n_seqs >= 0 && n_seqs + 1 <= cu_seqlens.numel(), op, ": n_seqs over the segments of cu_seqlens");
  SFT_CHECK(h.size(0) < (1L << 31), op, ": M over int32");
  SFT_CHECK(h.size(1) > 0 && h.size(1) % 8 == 0 && h.size(1) < (1L << 31), op, ": H must be a multiple of 8");
}

at::Tensor seq_score_fwd(const at::Tensor& h, const at::Tensor& w, const at::Tensor& cu_seqlens, int64_t n_seqs) {
  check_score_args("seq_score_fwd", h, w, cu_seqlens, n_seqs);
  auto out = at::empty({n_seqs}, h.options().dtype(at::kFloat));
  if (n_seqs == 0) return out;
  SFT_TRACE("reward.seq_score");
  seq_score_fwd_kernel<<<(unsigned)((n_seqs + 3) / 4), 256, 0, cur_stream()>>>(
      reinterpret_cast<const u16*>(h.data_ptr()), reinterpret_cast<const u16*>(w.data_ptr()),
      cu_seqlens.data_ptr<int>(), out.data_ptr<float>(), (int)n_seqs, (int)h.size(0), (int)h.size(1));
  SFT_LAUNCH_CHECK();
  return out;
}

// (dh bf16 [M, H], dw fp32 [H]); the half not asked for is an undefined tensor (None in Python) and launches nothing.
std::tuple<at::Tensor, at::Tensor> seq_score_bwd(const at::Tensor& g, const at::Tensor& h, const at::Tensor& w,
                                                 const at::Tensor& cu_seqlens, int64_t n_seqs, bool need_dh,
                                                 bool need_dw) {
  check_score_args("seq_score_bwd", h, w, cu_seqlens, n_seqs);
  SFT_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat && g.dim() == 1 && g.is_contiguous() && g.numel() == n_seqs &&
                g.get_device() == h.get_device(), "seq_score_bwd: g fp32 [n_seqs] on h's device");
  const int M = (int)h.size(0), H = (int)h.size(1);
  at::Tensor dh, dw;
  if (need_dh || need_dw) SFT_TRACE("reward.seq_score_bwd");
  if (need_dh) {
    dh = at::zeros_like(h);
    if (n_seqs > 0 && M > 0) {
      SFT_TRACE("reward.seq_score_bwd.dh");
      seq_score_dh_kernel<<<(unsigned)((n_seqs + 3) / 4), 256, 0, cur_stream()>>>(
          g.data_ptr<float>(), reinterpret_cast<const u16*>(w.data_ptr()), cu_seqlens.data_ptr<int>(),
          reinterpret_cast<u16*>(dh.data_ptr()), (int)n_seqs, M, H);
      SFT_LAUNCH_CHECK();
    }
  }
  if (need_dw) {
    dw = at::empty({(long)H}, h.options().dtype(at::kFloat));
    SFT_TRACE("reward.seq_score_bwd.dw");
    seq_score_dw_kernel<<<(unsigned)((H / 8 + 255) / 256), 256, 0, cur_stream()>>>(
        g.data_ptr<float>(), reinterpret_cast<const u16*>(h.data_ptr()), cu_seqlens.data_ptr<int>(),
        dw.data_ptr<float>(), (int)n_seqs, M, H);
    SFT_LAUNCH_CHECK();
  }
  return {dh, dw};
}

// Pair p = scores (2p chosen, 2p + 1 rejected), z = (r_c - r_r) - margin_p. stats [4, P]: the loss softplus(-z) + c
// (r_c + r_r)^2 (TRL RewardTrainer with center_rewards_coefficient c), d(inv_pairs sum loss) / d r_c, the same / d r_r,
// and z. With c == 0 the centring terms are not formed, so row 2 is the exact negation of row 1.
__global__ __launch_bounds__(256) void reward_pair_fwd_kernel(const float* __restrict__ scores,
                                                              const float* __restrict__ margins,
                                                              const float* __restrict__ inv_pairs,
                                                              float* __restrict__ stats, int P, float c) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float rc = scores[2 * p], rr = scores[2 * p + 1];
  const float m = margins != nullptr ? margins[p] : 0.f;
  const float z = (rc - rr) - m;
  float loss, sig;
  softplus_sigmoid_neg(z, loss, sig);
  const float inv = inv_pairs[0];
  float gc = -sig, gr = sig;
  if (c != 0.f) {
    const float sum = rc + rr;
    const float tc = (2.f * c) * sum;
    loss = loss + c * (sum * sum);
    gc = gc + tc;
    gr = gr + tc;
  }
  stats[p] = loss;
  stats[P + p] = gc * inv;
  stats[2 * P + p] = gr * inv;
  stats[3 * P + p] = z;
}

at::Tensor reward_pair_fwd(const at::Tensor& scores, const c10::optional<at::Tensor>& margins,
                           const at::Tensor& inv_pairs, double center_coef) {
  SFT_CHECK_CUDA(scores);
  SFT_CHECK(scores.scalar_type() == at::kFloat && scores.dim() == 1 && scores.is_contiguous() &&
                scores.numel() % 2 == 0, "reward_pair_fwd: scores fp32 [2 P]");
  const long P = scores.numel() / 2;
  const bool has_m = margins.has_value() && margins->defined();
  if (has_m)
    SFT_CHECK(margins->is_cuda() && margins->scalar_type() == at::kFloat && margins->is_contiguous() &&
                  margins->dim() == 1 && margins->numel() == P && margins->get_device() == scores.get_device(),
              "reward_pair_fwd: margins fp32 [P] on the scores' device");
  SFT_CHECK(inv_pairs.is_cuda() && inv_pairs.scalar_type() == at::kFloat && inv_pairs.numel() == 1 &&
                inv_pairs.get_device() == scores.get_device(), "reward_pair_fwd: inv_pairs a fp32 GPU scalar");
  SFT_CHECK(P < (1L << 28), "reward_pair_fwd: too many pairs");
  auto stats = at::empty({4, P}, scores.options());
  if (P == 0) return stats;
  SFT_TRACE("reward.pair");
  reward_pair_fwd_kernel<<<(unsigned)((P + 255) / 256), 256, 0, cur_stream()>>>(
      scores.data_ptr<float>(), has_m ? margins->data_ptr<float>() : nullptr, inv_pairs.data_ptr<float>(),
      stats.data_ptr<float>(), (int)P, (float)center_coef);
  SFT_LAUNCH_CHECK();
  return stats;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("seq_score_fwd", &seq_score_fwd);
  m.impl("seq_score_bwd", &seq_score_bwd);
  m.impl("reward_pair_fwd", &reward_pair_fwd);
}

}  // namespace sftamd
