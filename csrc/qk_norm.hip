// Per-head QK RMSNorm + RoPE on the packed qkv GEMM output (Qwen3: self_attn.q_norm / k_norm, weight [128] shared by
// all heads of a layer, applied after the projection and before the rotation), forward and backward, head_dim 128.
//
// Lane layout: 8 lanes per head row (qkv_rows.h); the row reductions (sum of squares, the backward's mean) stay inside
// the 8-lane group. A block (4 waves) covers 32 rows per grid-stride step; p is fixed per lane across steps, so the
// lane's 2 x 16 norm weights are loaded once. All math is fp32 with one rounding to bf16 at the store. No atomics.
//
// The forward keeps the un-normalised q|k columns (qk_raw) for the backward; rstd is NOT stored: the backward
// recomputes it from qk_raw, which it reads anyway (one more 3-step reduction instead of a [M, heads] tensor).
// The backward walks the query heads, then the key heads (one weight, one accumulator array per lane at a time).
// The weight gradients are reduced lane -> wave (shuffles over the 8 row groups) -> block (LDS, fixed order) into
// per-block fp32 partials [blocks, 2, 128]; an ordered second pass (two levels of 32) sums the blocks: bitwise
// reproducible.
#include "common.h"
#include "qkv_rows.h"

namespace sftamd {

constexpr int QN_D = 128;            // head_dim
constexpr int QN_ROWS = 32;          // rows per block per step (4 waves x 8 rows)
constexpr int QN_MAX_BLOCKS = 1024;  // 4 blocks / CU: 6 x 16 B in flight per lane saturate HBM; bounds the partials

static inline int qn_grid(long rows) {
  return (int)std::max<long>(1, std::min<long>((rows + QN_ROWS - 1) / QN_ROWS, QN_MAX_BLOCKS));
}

// raw: [M, nh * 128] copy of the un-normalised q|k columns (nullptr: not written — generation)
__global__ __launch_bounds__(256) void qk_norm_rope_fwd_kernel(u16* __restrict__ qkv, u16* __restrict__ raw,
                                                               const u16* __restrict__ qw, const u16* __restrict__ kw,
                                                               const float* __restrict__ cosb,
                                                               const float* __restrict__ sinb, int nrows, int ld,
                                                               int n_q, int nh, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (lane & 7) * 8;
  float wq[16], wk[16];
  unpack8(*(const uint4*)(qw + p), wq);
  unpack8(*(const uint4*)(qw + 64 + p), wq + 8);
  unpack8(*(const uint4*)(kw + p), wk);
  unpack8(*(const uint4*)(kw + 64 + p), wk + 8);
  // (the trip count is uniform over the block: the shuffles below run with every lane active)
  for (int base = blockIdx.x * QN_ROWS; base < nrows; base += gridDim.x * QN_ROWS) {
    const int r = base + wave * 8 + (lane >> 3);
    const bool ok = r < nrows;
    const int rc = ok ? r : nrows - 1;
    const int m = rc / nh, hh = rc - m * nh;
    u16* row = qkv + (long)m * ld + hh * QN_D + p;
    const uint4 va = *(const uint4*)row, vb = *(const uint4*)(row + 64);
    float c[8], s[8];
    load8f(cosb + (long)m * 64 + p, c);
    load8f(sinb + (long)m * 64 + p, s);
    float a[8], b[8];
    unpack8(va, a);
    unpack8(vb, b);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += a[i] * a[i] + b[i] * b[i];
    ss = group8_sum(ss);
    const float rstd = rsqrtf(ss * (1.f / QN_D) + eps);
    const bool isq = hh < n_q;
    float o1[8], o2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float n1 = (isq ? wq[i] : wk[i]) * (a[i] * rstd);
      const float n2 = (isq ? wq[8 + i] : wk[8 + i]) * (b[i] * rstd);
      rotate_pair_fwd(n1, n2, c[i], s[i], o1[i], o2[i]);
    }
    if (ok) {
      if (raw) {
        u16* rr = raw + (long)rc * QN_D + p;
        *(uint4*)rr = va;
        *(uint4*)(rr + 64) = vb;
      }
      *(uint4*)row = pack8(o1);
      *(uint4*)(row + 64) = pack8(o2);
    }
  }
}

// One head group (the query heads, or the key heads: heads h0 .. h0 + n of every token, norm weight w) of the backward:
// in place on dqkv, and this wave's column sums of g * xhat into red[128]. One weight array and one accumulator per
// lane live across the loop (the two groups as two passes keep the kernel at 4 waves / SIMD).
__device__ __forceinline__ void qn_bwd_group(u16* __restrict__ dqkv, const u16* __restrict__ raw,
                                             const u16* __restrict__ w, const float* __restrict__ cosb,
                                             const float* __restrict__ sinb, float* __restrict__ red, int M, int ld,
                                             int h0, int n, int nh, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (lane & 7) * 8;
  const int nrows = M * n;
  float wf[16], acc[16];
  unpack8(*(const uint4*)(w + p), wf);
  unpack8(*(const uint4*)(w + 64 + p), wf + 8);
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  // (the trip count is uniform over the block: the shuffles run with every lane active)
  for (int base = blockIdx.x * QN_ROWS; base < nrows; base += gridDim.x * QN_ROWS) {
    const int r = base + wave * 8 + (lane >> 3);
    const bool ok = r < nrows;
    const int rc = ok ? r : nrows - 1;
    const int m = rc / n, hh = h0 + (rc - m * n);
    u16* row = dqkv + (long)m * ld + hh * QN_D + p;
    const u16* rr = raw + ((long)m * nh + hh) * QN_D + p;
    const uint4 da = *(const uint4*)row, db = *(const uint4*)(row + 64);
    const uint4 xa = *(const uint4*)rr, xb = *(const uint4*)(rr + 64);
    float c[8], s[8];
    load8f(cosb + (long)m * 64 + p, c);
    load8f(sinb + (long)m * 64 + p, s);
    float d1[8], d2[8], xh[16];
    unpack8(da, d1);
    unpack8(db, d2);
    unpack8(xa, xh);
    unpack8(xb, xh + 8);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) ss += xh[i] * xh[i];
    ss = group8_sum(ss);
    const float rstd = rsqrtf(ss * (1.f / QN_D) + eps);
    // g: gradient w.r.t. the normalised, weighted row (the inverse rotation); gw = g w; xh = x rstd
    float g[16], gw[16];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) rotate_pair_inv(d1[i], d2[i], c[i], s[i], g[i], g[8 + i]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      xh[i] *= rstd;
      gw[i] = g[i] * wf[i];
      dot += gw[i] * xh[i];
    }
    dot = group8_sum(dot) * (1.f / QN_D);
    float o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o[i] = rstd * (gw[i] - xh[i] * dot);
      acc[i] += ok ? g[i] * xh[i] : 0.f;
    }
    if (ok) {
      *(uint4*)row = pack8(o);
      *(uint4*)(row + 64) = pack8(o + 8);
    }
  }
  wave_colsum128(acc, red, lane, p);
}

// dqkv: gradient w.r.t. the rotated q|k (in place -> gradient w.r.t. the raw q|k); part: [gridDim.x, 2, 128] fp32
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_kernel(u16* __restrict__ dqkv, const u16* __restrict__ raw,
                                                               const u16* __restrict__ qw, const u16* __restrict__ kw,
                                                               const float* __restrict__ cosb,
                                                               const float* __restrict__ sinb,
                                                               float* __restrict__ part, int M, int ld, int n_q,
                                                               int nh, float eps) {
  __shared__ float red[4][2][QN_D];
  const int wave = threadIdx.x >> 6;
  qn_bwd_group(dqkv, raw, qw, cosb, sinb, red[wave][0], M, ld, 0, n_q, nh, eps);
  qn_bwd_group(dqkv, raw, kw, cosb, sinb, red[wave][1], M, ld, n_q, nh - n_q, nh, eps);
  __syncthreads();
  const int t = threadIdx.x;  // 256 threads = 2 x 128 outputs
  const float* rp = &red[0][0][0];
  part[(long)blockIdx.x * 2 * QN_D + t] = ((rp[t] + rp[2 * QN_D + t]) + rp[4 * QN_D + t]) + rp[6 * QN_D + t];
}

// Ordered sum of partial rows: block g writes out[g, c] = sum of part[b, c] over b in [g * QN_FAN, (g + 1) * QN_FAN)
// (b < blocks), c in [0, 256). Slice j = 0..3 (one per 256 threads) takes rows j, j + 4, ... in order, all its (at
// most eight) loads in flight at once; the four slice sums are combined through LDS in a fixed order. Run twice
// (1024 -> 32 -> 1 rows) it is two short memory round trips instead of one block walking a thousand rows.
constexpr int QN_FAN = 32;

__global__ __launch_bounds__(1024) void qk_norm_dw_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                          int blocks) {
  __shared__ float red[4][256];
  const int c = threadIdx.x & 255, slice = threadIdx.x >> 8;
  part += (long)blockIdx.x * QN_FAN * 256;
  out += (long)blockIdx.x * 256;
  blocks = min(QN_FAN, blocks - (int)blockIdx.x * QN_FAN);
  float acc = 0.f;
  for (int b = slice; b < blocks; b += 32) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (b + 4 * k < blocks) ? part[(long)(b + 4 * k) * 256 + c] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  red[slice][c] = acc;
  __syncthreads();
  if (slice == 0) out[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

static void qn_check(const at::Tensor& qkv, const at::Tensor& qw, const at::Tensor& kw, const at::Tensor& cos,
                     const at::Tensor& sin, int64_t n_q, int64_t n_kv, int64_t head_dim, long& M, long& rows) {
  SFT_CHECK(head_dim == QN_D, "qk_norm_rope: head_dim must be 128");
  SFT_CHECK(n_q > 0 && n_kv > 0, "qk_norm_rope: head counts");
  M = check_qkv_rows("qk_norm_rope", qkv, cos, sin, n_q, n_kv, head_dim, true);
  SFT_CHECK_BF16(qw);
  SFT_CHECK_BF16(kw);
  SFT_CHECK(qw.is_cuda() && kw.is_cuda() && qw.is_contiguous() && kw.is_contiguous() && qw.numel() == QN_D &&
                kw.numel() == QN_D,
            "qk_norm_rope: norm weights must be contiguous bf16 [128] on the GPU");
  rows = M * (n_q + n_kv);
  SFT_CHECK(rows < (1L << 31) - (long)QN_MAX_BLOCKS * QN_ROWS, "qk_norm_rope: too many rows for 32-bit indexing");
  SFT_CHECK((((uintptr_t)qw.data_ptr() | (uintptr_t)kw.data_ptr()) & 15) == 0, "qk_norm_rope: 16-byte aligned weights");
}

at::Tensor qk_norm_rope_fwd(at::Tensor qkv, const at::Tensor& qw, const at::Tensor& kw, const at::Tensor& cos,
                            const at::Tensor& sin, int64_t n_q, int64_t n_kv, int64_t head_dim, double eps,
                            bool save_raw) {
  long M, rows;
  qn_check(qkv, qw, kw, cos, sin, n_q, n_kv, head_dim, M, rows);
  const int nh = n_q + n_kv;
  at::Tensor raw = save_raw ? at::empty({M, (long)nh * QN_D}, qkv.options()) : at::empty({0}, qkv.options());
  if (M == 0) return raw;
  SFT_TRACE("ew.qk_norm_rope.fwd");
  qk_norm_rope_fwd_kernel<<<qn_grid(rows), 256, 0, cur_stream()>>>(
      (u16*)qkv.data_ptr(), save_raw ? (u16*)raw.data_ptr() : nullptr, (const u16*)qw.data_ptr(),
      (const u16*)kw.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), (int)rows, (int)qkv.size(-1), (int)n_q,
      nh, (float)eps);
  SFT_LAUNCH_CHECK();
  return raw;
}

std::tuple<at::Tensor, at::Tensor> qk_norm_rope_bwd(at::Tensor dqkv, const at::Tensor& raw, const at::Tensor& qw,
                                                    const at::Tensor& kw, const at::Tensor& cos, const at::Tensor& sin,
                                                    int64_t n_q, int64_t n_kv, int64_t head_dim, double eps) {
  long M, rows;
  qn_check(dqkv, qw, kw, cos, sin, n_q, n_kv, head_dim, M, rows);
  const int nh = n_q + n_kv;
  SFT_CHECK_CUDA(raw);
  SFT_CHECK_BF16(raw);
  SFT_CHECK_CONTIG(raw);
  SFT_CHECK(raw.numel() == rows * QN_D && ((uintptr_t)raw.data_ptr() & 15) == 0, "qk_norm_rope_bwd: qk_raw shape");
  auto fopt = dqkv.options().dtype(at::kFloat);
  auto dw = M == 0 ? at::zeros({2, QN_D}, fopt) : at::empty({2, QN_D}, fopt);
  if (M == 0) return {dw[0], dw[1]};
  const int grid = qn_grid(rows);
  auto part = at::empty({grid, 2, QN_D}, fopt);
  SFT_TRACE("ew.qk_norm_rope.bwd");
  qk_norm_rope_bwd_kernel<<<grid, 256, 0, cur_stream()>>>(
      (u16*)dqkv.data_ptr(), (const u16*)raw.data_ptr(), (const u16*)qw.data_ptr(), (const u16*)kw.data_ptr(),
      cos.data_ptr<float>(), sin.data_ptr<float>(), part.data_ptr<float>(), (int)M, (int)dqkv.size(-1), (int)n_q, nh,
      (float)eps);
  SFT_LAUNCH_CHECK();
  static_assert(QN_MAX_BLOCKS <= QN_FAN * QN_FAN, "two levels of the ordered sum cover every grid");
  const float* src = part.data_ptr<float>();
  int n = grid;
  at::Tensor mid;
  if (n > QN_FAN) {
    const int g2 = (n + QN_FAN - 1) / QN_FAN;
    mid = at::empty({g2, 2, QN_D}, fopt);
    qk_norm_dw_kernel<<<g2, 1024, 0, cur_stream()>>>(src, mid.data_ptr<float>(), n);
    SFT_LAUNCH_CHECK();
    src = mid.data_ptr<float>();
    n = g2;
  }
  qk_norm_dw_kernel<<<1, 1024, 0, cur_stream()>>>(src, dw.data_ptr<float>(), n);
  SFT_LAUNCH_CHECK();
  return {dw[0], dw[1]};
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("qk_norm_rope_fwd", &qk_norm_rope_fwd);
  m.impl("qk_norm_rope_bwd", &qk_norm_rope_bwd);
}

}  // namespace sftamd
