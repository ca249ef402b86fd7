// Fused knowledge-distillation loss over a 128k vocabulary for gfx950: the generalized Jensen-Shannon divergence of
// TRL's GKDTrainer between a student's and a teacher's bf16 logits (twin: ops/reference.py generalized_jsd).
//
// One 256-thread block per token row; the accumulator (RowAcc, its t = the KL numerator sum e^(x-m) d, d = x - the other
// row's value) with its merge, the row sweep and the rows-in-flight cap are vocab_rows.h's, shared with ce_fwd; the block
// combine follows the order given there, for two accumulators at once. With a = s / tau, b = t / tau,
// lp = a - lse(a), lq = b - lse(b), p = e^lp, q = e^lq, per valid row:
//   KD_FKL (beta 0)  L = sum q (lq - lp)                                   dL/da_i = p_i - q_i
//   KD_RKL (beta 1)  L = sum p (lp - lq)                                   dL/da_i = p_i ((lp_i - lq_i) - L)
//   KD_MIX           lm = logsumexp(lp + log(1 - beta), lq + log beta),    dL/da_i = (1 - beta) p_i ((lp_i - lm_i) - K),
//                    L = beta sum q (lq - lm) + (1 - beta) sum p (lp - lm)           K = sum p (lp - lm)
// Pass 1 streams both rows once with 16-byte loads and keeps, per thread, an online (max, sum e^(x-max), argmax) of
// each row plus the KL numerator its mode needs (KD_FKL: sum e^(b-m_t) (b - a); KD_RKL: sum e^(a-m_s) (a - b)), so the
// two KL modes know their loss and their gradient's scalar after one pass: L = numerator / sum + (lse - lse'). KD_MIX
// takes a second pass for its two sums once both lse are known. The gradient pass overwrites the STUDENT's row in
// place with bf16 dL/ds_i = dL/da_i * inv_count / tau; the teacher's row is only read. Everything stays in the log
// domain (no log of a probability), so finite logits give a finite loss and gradient while their gap fits fp32.
// The mode is a template parameter: the mixture's extra transcendentals are not in the two KL instantiations.
#include "vocab_rows.h"

#include <cmath>
#include <cstdlib>

namespace sftamd {

constexpr int KD_FKL = 0, KD_RKL = 1, KD_MIX = 2;

// Eight elements x of one row (columns base .. base + 7, visited in increasing order by a thread) into its online
// accumulator: one rescale of the running sums when the maximum moves (e^(-inf) = 0 on the first vector), then the
// eight terms against the new maximum. NUM: also the KL numerator, sign * (xa - xb).
template <bool NUM>
__device__ __forceinline__ void kd_accum(RowAcc& acc, const float* x, const float* xa, const float* xb, int base) {
  float mx = x[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) mx = fmaxf(mx, x[i]);
  const float M = fmaxf(acc.m, mx);
  const float sc = __expf(acc.m - M);
  float s = 0.f, r = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float e = __expf(x[i] - M);
    s += e;
    if constexpr (NUM) r += e * (xa[i] - xb[i]);
    if (x[i] > acc.bv) {
      acc.bv = x[i];
      acc.bi = base + i;
    }
  }
  acc.s = acc.s * sc + s;
  if constexpr (NUM) acc.t = acc.t * sc + r;
  acc.m = M;
}

template <int KD_U, int MODE>  // row loads in flight per thread and row, objective
__global__ __launch_bounds__(256) void kd_fwd_kernel(u16* __restrict__ student, const u16* __restrict__ teacher,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ inv_count, float* __restrict__ stats,
                                                     int M, int V, int write_grad, float beta, float log_beta,
                                                     float log_1mbeta, float inv_tau) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  u16* sr = student + (long)row * V;
  const u16* tr = teacher + (long)row * V;
  const long label = labels[row];
  SFT_DASSERT(label == -100 || (label >= 0 && label < V));
  const bool valid = label >= 0 && label < V;
  const int nvec = V / 8;

  auto sweep = [&](auto&& body) { sweep_row_pair<KD_U>(sr, tr, nvec, tid, body); };
  auto scaled = [&](const uint4& raw, float* x) {
    unpack8(raw, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] *= inv_tau;
  };

  // ---- pass 1: online (max, sum, argmax) of both rows and the mode's KL numerator
  RowAcc as = row_acc_empty(), at = row_acc_empty();
  sweep([&](const uint4& rs, const uint4& rt, int v) {
    float a[8], b[8];
    scaled(rs, a);
    scaled(rt, b);
    kd_accum<MODE == KD_RKL>(as, a, a, b, v * 8);
    kd_accum<MODE == KD_FKL>(at, b, b, a, v * 8);
  });
  // the block combine in the order vocab_rows.h gives, for two accumulators
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    row_merge(as, row_shfl_xor(as, o));
    row_merge(at, row_shfl_xor(at, o));
  }
  __shared__ RowAcc red_s[4], red_t[4];
  __shared__ float red_kp[4], red_kq[4];  // KD_MIX: the waves' two mixture sums
  __shared__ float sh_lse_s, sh_lse_t, sh_c;  // sh_c: the gradient's row scalar (KD_RKL: L, KD_MIX: K)
  if ((tid & 63) == 0) {
    red_s[tid >> 6] = as;
    red_t[tid >> 6] = at;
  }
  __syncthreads();
  if (tid == 0) {
    RowAcc a = red_s[0], b = red_t[0];
    for (int w = 1; w < 4; ++w) {
      row_merge(a, red_s[w]);
      row_merge(b, red_t[w]);
    }
    const float lse_s = a.m + __logf(a.s);
    const float lse_t = b.m + __logf(b.s);
    if constexpr (MODE == KD_FKL) stats[row] = valid ? (b.t / b.s + (lse_s - lse_t)) : 0.f;
    if constexpr (MODE == KD_RKL) {
      const float L = a.t / a.s + (lse_t - lse_s);
      stats[row] = valid ? L : 0.f;
      sh_c = L;
    }
    if constexpr (MODE == KD_MIX) {
      if (!valid) stats[row] = 0.f;
    }
    stats[M + row] = lse_s;
    stats[2 * M + row] = lse_t;
    stats[3 * M + row] = (valid && a.bi == label) ? 1.f : 0.f;
    stats[4 * M + row] = (valid && a.bi == b.bi) ? 1.f : 0.f;
    sh_lse_s = lse_s;
    sh_lse_t = lse_t;
  }
  __syncthreads();
  const float lse_s = sh_lse_s, lse_t = sh_lse_t;

  // ---- the mixture's pass: both KL sums against lm, in the log domain
  auto log_mix = [&](float lp, float lq) {  // logsumexp(lp + log(1 - beta), lq + log beta)
    const float u = lp + log_1mbeta, w = lq + log_beta;
    return fmaxf(u, w) + __logf(1.f + __expf(-fabsf(u - w)));
  };
  if constexpr (MODE == KD_MIX) {
    if (valid) {
      float kp = 0.f, kq = 0.f;
      sweep([&](const uint4& rs, const uint4& rt, int) {
        float a[8], b[8];
        scaled(rs, a);
        scaled(rt, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float lp = a[i] - lse_s, lq = b[i] - lse_t;
          const float lm = log_mix(lp, lq);
          kp += __expf(lp) * (lp - lm);
          kq += __expf(lq) * (lq - lm);
        }
      });
      kp = wave_sum(kp);
      kq = wave_sum(kq);
      if ((tid & 63) == 0) {
        red_kp[tid >> 6] = kp;
        red_kq[tid >> 6] = kq;
      }
      __syncthreads();
      if (tid == 0) {
        const float KP = (red_kp[0] + red_kp[1]) + (red_kp[2] + red_kp[3]);
        const float KQ = (red_kq[0] + red_kq[1]) + (red_kq[2] + red_kq[3]);
        stats[row] = beta * KQ + (1.f - beta) * KP;
        sh_c = KP;
      }
      __syncthreads();
    }
  }
  if (!write_grad) return;

  // ---- gradient pass: the student's row becomes dL/ds * inv_count (a label-masked row: +0 in every element)
  if (!valid) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int v = tid; v < nvec; v += 256) *(uint4*)(sr + (long)v * 8) = zero;
    return;
  }
  const float c = MODE == KD_FKL ? 0.f : sh_c;
  float scale = inv_count[0] * inv_tau;
  if constexpr (MODE == KD_MIX) scale *= 1.f - beta;
  sweep([&](const uint4& rs, const uint4& rt, int v) {
    float a[8], b[8];
    scaled(rs, a);
    scaled(rt, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float lp = a[i] - lse_s, lq = b[i] - lse_t;
      if constexpr (MODE == KD_FKL) a[i] = (__expf(lp) - __expf(lq)) * scale;
      if constexpr (MODE == KD_RKL) a[i] = (__expf(lp) * ((lp - lq) - c)) * scale;
      if constexpr (MODE == KD_MIX) a[i] = (__expf(lp) * ((lp - log_mix(lp, lq)) - c)) * scale;
    }
    *(uint4*)(sr + (long)v * 8) = pack8(a);
  });
}

template <int MODE>
static void kd_launch(u16* st, const u16* te, const int64_t* lab, const float* inv, float* stats, int M, int V,
                      bool write_grad, float beta, float inv_tau, int pad) {
  allow_row_pad<kd_fwd_kernel<4, MODE>>(pad, "kd_fwd");
  const float lb = MODE == KD_MIX ? (float)std::log((double)beta) : 0.f;
  const float l1 = MODE == KD_MIX ? (float)std::log1p(-(double)beta) : 0.f;
  kd_fwd_kernel<4, MODE><<<M, 256, pad, cur_stream()>>>(st, te, lab, inv, stats, M, V, write_grad ? 1 : 0, beta, lb,
                                                        l1, inv_tau);
}

// Rows in flight while the gradient is written, in MB (see kd_fwd): SFTAMD_KD_INFLIGHT_MB overrides the default
// (tools/bench_kd.py measures with it).
static long kd_inflight_mb() {
  static long mb = [] {
    const char* e = std::getenv("SFTAMD_KD_INFLIGHT_MB");
    const long v = e && e[0] ? std::atol(e) : 0;
    return v > 0 ? v : 300L;
  }();
  return mb;
}

at::Tensor kd_fwd(at::Tensor student_logits, const at::Tensor& teacher_logits, const at::Tensor& labels,
                  const at::Tensor& inv_count, bool write_grad, double beta, double temperature) {
  SFT_CHECK_CUDA(student_logits);
  SFT_CHECK_CUDA(teacher_logits);
  SFT_CHECK_BF16(student_logits);
  SFT_CHECK_BF16(teacher_logits);
  SFT_CHECK_CONTIG(student_logits);
  SFT_CHECK_CONTIG(teacher_logits);
  SFT_CHECK(student_logits.dim() >= 1 && student_logits.sizes() == teacher_logits.sizes(),
            "kd_fwd: student and teacher logits must have the same shape");
  SFT_CHECK(student_logits.device() == teacher_logits.device(), "kd_fwd: logits on two devices");
  SFT_CHECK(labels.scalar_type() == at::kLong && labels.is_cuda(), "labels must be an int64 GPU tensor");
  SFT_CHECK(inv_count.scalar_type() == at::kFloat && inv_count.is_cuda() && inv_count.numel() >= 1,
            "inv_count must be a fp32 GPU tensor");
  SFT_CHECK(beta >= 0.0 && beta <= 1.0, "kd_fwd: beta must be in [0, 1]");
  SFT_CHECK(temperature > 0.0 && std::isfinite(temperature), "kd_fwd: temperature must be > 0");
  const long Vl = student_logits.size(-1);
  SFT_CHECK(Vl > 0 && Vl % 8 == 0 && Vl <= INT_MAX, "vocab must be a multiple of 8");
  const int V = (int)Vl;
  const long Ml = student_logits.numel() / V;
  SFT_CHECK(Ml <= INT_MAX / 5, "kd_fwd: too many rows");
  const int M = (int)Ml;
  SFT_CHECK(labels.numel() == M, "labels size");
  auto lab = labels.contiguous();
  auto stats = at::empty({5, M}, student_logits.options().dtype(at::kFloat));
  if (M == 0) return stats;
  SFT_CHECK(student_logits.data_ptr() != teacher_logits.data_ptr(),
            "kd_fwd: the teacher's logits must not alias the student's (the gradient is written over the student's)");
  // The rows-in-flight cap (vocab_rows.h) with the doubled row: the gradient pass (and the mixture's pass) re-read both
  // rows. ce_fwd's 200 MB leaves ONE block per CU at V = 128,256 (a row pair is 513 KB), too few waves to cover the load
  // latency; 300 MB (two blocks, 263 MB in flight) is the fastest of 200 / 300 / 400 / 540 / uncapped at 8192 rows:
  // 1.78 vs 1.96 / 1.96 / 1.98 / 1.98 ms forward KL, 2.51 vs 3.14 / 2.51 / 2.77 / 2.77 ms mixture
  // (tools/bench_kd.py, profiles/distill.md). The stats-only call (eval) keeps full occupancy.
  const int pad = write_grad ? rows_in_flight_pad(2L * V * 2, kd_inflight_mb()) : 0;
  auto* sp = (u16*)student_logits.data_ptr();
  auto* tp = (const u16*)teacher_logits.data_ptr();
  auto* lb = lab.data_ptr<int64_t>();
  auto* ic = inv_count.data_ptr<float>();
  auto* st = stats.data_ptr<float>();
  const float inv_tau = (float)(1.0 / temperature);
  if (beta == 0.0) {
    SFT_TRACE("kd_fwd.fkl");
    kd_launch<KD_FKL>(sp, tp, lb, ic, st, M, V, write_grad, 0.f, inv_tau, pad);
  } else if (beta == 1.0) {
    SFT_TRACE("kd_fwd.rkl");
    kd_launch<KD_RKL>(sp, tp, lb, ic, st, M, V, write_grad, 1.f, inv_tau, pad);
  } else {
    SFT_TRACE("kd_fwd.mix");
    kd_launch<KD_MIX>(sp, tp, lb, ic, st, M, V, write_grad, (float)beta, inv_tau, pad);
  }
  SFT_LAUNCH_CHECK();
  return stats;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) { m.impl("kd_fwd", &kd_fwd); }

}  // namespace sftamd
