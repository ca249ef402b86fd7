// Fused cross-entropy over a 128k vocabulary for gfx950.
//
// One 256-thread block per token row. Pass 1 streams the bf16 logits row once with 16-byte
// loads and keeps an online (max, sum e^(x-max), sum e^(x-max)*x, argmax) per thread; the
// block combines them to get logsumexp, the per-token loss, the entropy and the argmax
// accuracy bit (the TRL training metrics, at no extra pass). Pass 2 re-reads the row (L2 /
// Infinity-Cache resident: the launch caps the rows in flight, see ce_fwd) and overwrites it IN PLACE with the bf16 gradient
// (softmax - onehot) * (1/num_items_in_batch): fp32 logits are never materialised.
//
// The objective is a template parameter (CE_NLL / CE_SMOOTH / CE_DFT / CE_TEMP below): label smoothing adds one fp32
// sum(x) accumulator to pass 1, DFT one weight broadcast through LDS, the temperature one fp32 multiply per loaded
// logit; the plain instantiation keeps its loop bodies.
//
// The accumulator (RowAcc, its t = sum e^(x-max)*x) with its merge and shuffle, and the rows-in-flight cap, are
// vocab_rows.h's; the per-vector accumulation, the row loops and the gradient expression are this file's.
#include "vocab_rows.h"

namespace sftamd {

// Objectives, per valid row (x the bf16 logits, y the label, p = softmax(x), s = inv_count):
//   CE_NLL     loss = lse - x_y                          dlogit_i = (p_i - [i == y]) s
//   CE_SMOOTH  loss = lse - (1 - e) x_y - e sum(x) / V   dlogit_i = (p_i - (1 - e) [i == y] - e / V) s   (HF LabelSmoother)
//   CE_DFT     loss = w (lse - x_y), w = p_y constant    dlogit_i = w (p_i - [i == y]) s                 (TRL dft_loss)
//   CE_TEMP    CE_NLL of z = x / tau (z_i = x_i * (1 / tau) in fp32, in both passes and for the label's logit): lse,
//              entropy and the argmax bit are those of softmax(z); the buffer receives (softmax(z)_i - [i == y]) s,
//              WITHOUT the chain rule's 1 / tau, which the caller puts onto its row weight (csrc/policy.hip)
constexpr int CE_NLL = 0, CE_SMOOTH = 1, CE_DFT = 2, CE_TEMP = 3;

template <int CE_U, int MODE>  // row loads in flight per thread, objective
__global__ __launch_bounds__(256) void ce_fwd_kernel(u16* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ inv_count, float* __restrict__ stats,
                                                     int M, int V, int write_grad, float smooth) {  // (CE_TEMP: smooth carries 1 / tau)
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  u16* lr = logits + (long)row * V;
  const long label = labels[row];
  SFT_DASSERT(label == -100 || (label >= 0 && label < V));
  const bool valid = label >= 0 && label < V;
  const int nvec = V / 8;

  RowAcc acc = row_acc_empty();
  float sumx = 0.f;  // CE_SMOOTH: sum of the row's logits
  auto accum = [&](const uint4& raw, int v) {
    float x[8];
    unpack8(raw, x);
    if constexpr (MODE == CE_TEMP) {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] *= smooth;
    }
    float mx = x[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) mx = fmaxf(mx, x[i]);
    RowAcc b{mx, 0.f, 0.f, -INFINITY, INT_MAX};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float e = __expf(x[i] - mx);
      b.s += e;
      b.t += e * x[i];
      if (x[i] > b.bv) {
        b.bv = x[i];
        b.bi = v * 8 + i;
      }
    }
    if constexpr (MODE == CE_SMOOTH) {
      float sv = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) sv += x[i];
      sumx += sv;
    }
    row_merge(acc, b);
  };
  // U independent 16-byte loads in flight per thread before any of them is consumed: one load per iteration
  // leaves the row stream latency-bound (~3.5 TB/s); ties in the argmax resolve by index in row_merge, so the
  // visiting order does not change the result
  int v = tid;
  for (; v + 256 * (CE_U - 1) < nvec; v += 256 * CE_U) {
    uint4 r[CE_U];
#pragma unroll
    for (int u = 0; u < CE_U; ++u) r[u] = *(const uint4*)(lr + (long)(v + 256 * u) * 8);
#pragma unroll
    for (int u = 0; u < CE_U; ++u) accum(r[u], v + 256 * u);
  }
  for (; v < nvec; v += 256) accum(*(const uint4*)(lr + (long)v * 8), v);
  // block combine: the xor butterfly per wave, then waves 0..3 in order through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) row_merge(acc, row_shfl_xor(acc, o));
  __shared__ RowAcc red[4];
  __shared__ float sh_lse;
  __shared__ float red_sx[4];  // CE_SMOOTH: the waves' sum(x)
  __shared__ float sh_w;       // CE_DFT: the row's weight p_y
  if constexpr (MODE == CE_SMOOTH) sumx = wave_sum(sumx);
  if ((tid & 63) == 0) {
    red[tid >> 6] = acc;
    if constexpr (MODE == CE_SMOOTH) red_sx[tid >> 6] = sumx;
  }
  __syncthreads();
  if (tid == 0) {
    RowAcc a = red[0];
    for (int w = 1; w < 4; ++w) row_merge(a, red[w]);
    const float lse = a.m + __logf(a.s);
    float xl = valid ? bf2f(lr[label]) : 0.f;
    if constexpr (MODE == CE_TEMP) xl *= smooth;
    if constexpr (MODE == CE_SMOOTH) {
      const float sx = (red_sx[0] + red_sx[1]) + (red_sx[2] + red_sx[3]);
      stats[row] = valid ? (lse - (1.f - smooth) * xl - smooth * (sx / (float)V)) : 0.f;
    } else if constexpr (MODE == CE_DFT) {
      const float w = valid ? __expf(xl - lse) : 0.f;
      stats[row] = w * (lse - xl);
      sh_w = w;
    } else {
      stats[row] = valid ? (lse - xl) : 0.f;
    }
    stats[M + row] = lse;
    stats[2 * M + row] = lse - a.t / a.s;
    stats[3 * M + row] = (valid && a.bi == label) ? 1.f : 0.f;
    sh_lse = lse;
  }
  __syncthreads();
  if (!write_grad) return;
  const float lse = sh_lse;
  float scale = valid ? inv_count[0] : 0.f;
  if constexpr (MODE == CE_DFT) scale *= sh_w;
  const float hot = MODE == CE_SMOOTH ? 1.f - smooth : 1.f;   // weight of the label's column
  const float flat = MODE == CE_SMOOTH ? smooth / (float)V : 0.f;  // CE_SMOOTH: weight of every column
  auto grad = [&](const uint4& raw, int v) {
    float x[8];
    unpack8(raw, x);
    if constexpr (MODE == CE_TEMP) {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] *= smooth;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float p = __expf(x[i] - lse);
      if constexpr (MODE == CE_SMOOTH)
        x[i] = ((p - ((v * 8 + i) == label ? hot : 0.f)) - flat) * scale;
      else
        x[i] = (p - ((v * 8 + i) == label ? 1.f : 0.f)) * scale;
    }
    *(uint4*)(lr + (long)v * 8) = pack8(x);
  };
  v = tid;
  for (; v + 256 * (CE_U - 1) < nvec; v += 256 * CE_U) {
    uint4 r[CE_U];
#pragma unroll
    for (int u = 0; u < CE_U; ++u) r[u] = *(const uint4*)(lr + (long)(v + 256 * u) * 8);
#pragma unroll
    for (int u = 0; u < CE_U; ++u) grad(r[u], v + 256 * u);
  }
  for (; v < nvec; v += 256) grad(*(const uint4*)(lr + (long)v * 8), v);
}

template <int MODE>
static void ce_launch(u16* lg, const int64_t* lab, const float* inv, float* stats, int M, int V, bool write_grad,
                      float smooth, int pad) {
  allow_row_pad<ce_fwd_kernel<4, MODE>>(pad, "ce_fwd");
  ce_fwd_kernel<4, MODE><<<M, 256, pad, cur_stream()>>>(lg, lab, inv, stats, M, V, write_grad ? 1 : 0, smooth);
}

at::Tensor ce_fwd(at::Tensor logits, const at::Tensor& labels, const at::Tensor& inv_count, bool write_grad,
                  double label_smoothing, int64_t loss_mode, double temperature) {
  SFT_CHECK_BF16(logits);
  SFT_CHECK_CONTIG(logits);
  SFT_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  SFT_CHECK(inv_count.scalar_type() == at::kFloat && inv_count.is_cuda(), "inv_count must be a fp32 GPU tensor");
  SFT_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0, "ce_fwd: label_smoothing must be in [0, 1)");
  SFT_CHECK(loss_mode == 0 || loss_mode == 1, "ce_fwd: loss_mode 0 (nll) or 1 (dft)");
  SFT_CHECK(loss_mode == 0 || label_smoothing == 0.0, "ce_fwd: dft takes no label smoothing");
  SFT_CHECK(temperature > 0.0, "ce_fwd: temperature must be > 0");
  SFT_CHECK(temperature == 1.0 || (label_smoothing == 0.0 && loss_mode == 0),
            "ce_fwd: a temperature takes neither label smoothing nor dft");
  const int V = logits.size(-1);
  const int M = logits.numel() / V;
  SFT_CHECK(V % 8 == 0, "vocab must be a multiple of 8");
  SFT_CHECK(labels.numel() == M, "labels size");
  auto lab = labels.contiguous();
  auto stats = at::empty({4, M}, logits.options().dtype(at::kFloat));
  if (M == 0) return stats;
  auto* lg = (u16*)logits.data_ptr();
  // The rows-in-flight cap (vocab_rows.h): with 8 blocks per CU the SmolLM3 bench's 2048 rows x 256 KB = 512 MB of rows
  // in flight overflow the 256 MB cache and pass 2 goes back to HBM. With the gradient written the budget is 200 MB:
  // 3 blocks per CU at V = 128,256 — 1.037 vs 1.227 ms per call at 8192 rows (tools/bench_ce.py,
  // profiles/r6_memory_kernels.md), 2 above ~136K (a 79 KB pad at 151,936, 159 KB at 262,144); the stats-only pass
  // (eval) keeps full occupancy.
  const int pad = write_grad ? rows_in_flight_pad((long)V * 2, 200) : 0;
  auto* lb = lab.data_ptr<int64_t>();
  auto* ic = inv_count.data_ptr<float>();
  auto* st = stats.data_ptr<float>();
  if (temperature != 1.0) {
    SFT_TRACE("ce.temp");
    ce_launch<CE_TEMP>(lg, lb, ic, st, M, V, write_grad, (float)(1.0 / temperature), pad);
  } else if (loss_mode == 1) ce_launch<CE_DFT>(lg, lb, ic, st, M, V, write_grad, 0.f, pad);
  else if (label_smoothing > 0.0) ce_launch<CE_SMOOTH>(lg, lb, ic, st, M, V, write_grad, (float)label_smoothing, pad);
  else ce_launch<CE_NLL>(lg, lb, ic, st, M, V, write_grad, 0.f, pad);
  SFT_LAUNCH_CHECK();
  return stats;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) { m.impl("ce_fwd", &ce_fwd); }

}  // namespace sftamd
