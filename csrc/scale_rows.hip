// The row weight of the LM-head objectives' backward, for gfx950: a per-row weight commutes with both backward GEMMs
// (dh = diag(r) (G W), dW = G^T (diag(r) h)), so it goes onto the two [T, hidden] operands, never onto the [T, vocab]
// one. One kernel, two forms: scale_rows takes one weight per row (the GRPO policy loss), scale_rows_by_seq one per
// sequence of cu_seqlens (sequence log-probabilities, DPO).
#include "common.h"

#include <algorithm>

namespace sftamd {

// out[t, :] = bf16(float(x[t, :]) * (coef[r] * gscale)), r = t, or with BY_SEQ the segment s(t) of row t; rows at or
// past cu[n_seqs]: +0. blockIdx.y strides the rows (M may pass the grid's 65535), so the row and its segment search
// (over cu[1 .. n_seqs]) are uniform in the block: once per row, scalar loads. x and out may be the same buffer (the
// in-place form): every vector is read before it is written, by the thread that writes it.
template <bool BY_SEQ>
__global__ __launch_bounds__(256) void scale_rows_kernel(const u16* x, u16* out, const float* __restrict__ coef,
                                                         const int* __restrict__ cu, const float* __restrict__ gscale,
                                                         long M, int H, int n_seqs) {
  const int k = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (k >= H) return;
  const float g = gscale[0];
  for (long t = blockIdx.y; t < M; t += gridDim.y) {
    int lo = 0;  // BY_SEQ: the number of boundaries cu[1 .. n_seqs] at or below t
    if constexpr (BY_SEQ) {
      int hi = n_seqs;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)cu[mid + 1] <= t) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= n_seqs) {
        *(uint4*)(out + t * H + k) = make_uint4(0u, 0u, 0u, 0u);
        continue;
      }
    }
    const float c = (BY_SEQ ? coef[lo] : coef[t]) * g;
    float v[8];
    unpack8(*(const uint4*)(x + t * H + k), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] *= c;
    *(uint4*)(out + t * H + k) = pack8(v);
  }
}

// cu == nullptr: one weight per row (scale_rows); else one per segment (scale_rows_by_seq). ``op`` names the caller in
// the messages.
static void scale_rows_launch(const char* op, const at::Tensor& x, at::Tensor& out, const at::Tensor& coef,
                              const at::Tensor* cu, int64_t n_seqs, const at::Tensor& gscale) {
  SFT_CHECK_CUDA(x);
  SFT_CHECK_BF16(x);
  SFT_CHECK_CONTIG(x);
  SFT_CHECK(x.dim() == 2 && x.size(1) % 8 == 0, op, ": x [M, H], H a multiple of 8");
  SFT_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat && coef.is_contiguous() &&
                (cu ? coef.numel() == n_seqs : coef.dim() == 1 && coef.numel() == x.size(0)),
            op, cu ? ": coef fp32 [n_seqs] on the GPU" : ": coef fp32 [M] on the GPU");
  if (cu) {
    SFT_CHECK(cu->is_cuda() && cu->scalar_type() == at::kInt && cu->dim() == 1 && cu->is_contiguous(), op,
              ": cu_seqlens int32 [S + 1] on the GPU");
    SFT_CHECK(n_seqs >= 0 && n_seqs + 1 <= cu->numel(), op, ": n_seqs over the segments of cu_seqlens");
  }
  SFT_CHECK(gscale.is_cuda() && gscale.scalar_type() == at::kFloat && gscale.numel() == 1, op,
            ": gscale a fp32 GPU scalar");
  const long M = x.size(0);
  const int H = x.size(1);
  if (M == 0 || H == 0) return;
  dim3 grid((H / 8 + 255) / 256, (unsigned)std::min<long>(M, 65535));
  auto* xp = (const u16*)x.data_ptr();
  auto* yp = (u16*)out.data_ptr();
  if (cu) {
    SFT_TRACE("pref.scale_rows");
    scale_rows_kernel<true><<<grid, 256, 0, cur_stream()>>>(xp, yp, coef.data_ptr<float>(), cu->data_ptr<int>(),
                                                            gscale.data_ptr<float>(), M, H, (int)n_seqs);
  } else {
    SFT_TRACE("policy.scale_rows");
    scale_rows_kernel<false><<<grid, 256, 0, cur_stream()>>>(xp, yp, coef.data_ptr<float>(), nullptr,
                                                             gscale.data_ptr<float>(), M, H, 0);
  }
  SFT_LAUNCH_CHECK();
}

at::Tensor scale_rows(const at::Tensor& x, const at::Tensor& coef, const at::Tensor& gscale) {
  SFT_CHECK_CUDA(x);
  auto out = at::empty_like(x);
  scale_rows_launch("scale_rows", x, out, coef, nullptr, 0, gscale);
  return out;
}

void scale_rows_(at::Tensor x, const at::Tensor& coef, const at::Tensor& gscale) {
  scale_rows_launch("scale_rows", x, x, coef, nullptr, 0, gscale);
}

at::Tensor scale_rows_by_seq(const at::Tensor& x, const at::Tensor& coef, const at::Tensor& cu_seqlens, int64_t n_seqs,
                             const at::Tensor& gscale) {
  SFT_CHECK_CUDA(x);
  auto out = at::empty_like(x);
  scale_rows_launch("scale_rows_by_seq", x, out, coef, &cu_seqlens, n_seqs, gscale);
  return out;
}

void scale_rows_by_seq_(at::Tensor x, const at::Tensor& coef, const at::Tensor& cu_seqlens, int64_t n_seqs,
                        const at::Tensor& gscale) {
  scale_rows_launch("scale_rows_by_seq", x, x, coef, &cu_seqlens, n_seqs, gscale);
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("scale_rows", &scale_rows);
  m.impl("scale_rows_", &scale_rows_);
  m.impl("scale_rows_by_seq", &scale_rows_by_seq);
  m.impl("scale_rows_by_seq_", &scale_rows_by_seq_);
}

}  // namespace sftamd
