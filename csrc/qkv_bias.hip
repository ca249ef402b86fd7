// Learned bias on the q, k and v projections + RoPE on the packed qkv GEMM output (Qwen2 / Qwen2.5:
// self_attn.{q,k,v}_proj.bias, added after the projection and before the rotation), forward and backward, head_dim 128.
//
// Lane layout: 8 lanes per head row (qkv_rows.h). The head is fixed per block (blockIdx.y) and the block strides
// over tokens, 32 per step (4 waves x 8 rows), so a lane's 16 columns never change: its 16 bias values are loaded
// once, and the backward keeps 16 fp32 column sums in registers. Whether the block's head is rotated (q, k) or only
// biased (v) is uniform over the block. All math is fp32 with one rounding to bf16 at the store. No atomics.
//
// The node is linear, so the forward keeps nothing. The backward un-rotates the q|k columns of the gradient in place
// (the v columns are read, never written) and sums every column over the tokens: lane -> wave (shuffles over the 8
// row groups) -> block (LDS, fixed order) into fp32 partials [gridDim.x, heads * 128]; a second kernel adds the
// partial rows in order: bitwise reproducible. gridDim.x * heads <= 1024 bounds the partials (512 KB).
#include "common.h"
#include "qkv_rows.h"

namespace sftamd {

constexpr int QB_D = 128;            // head_dim
constexpr int QB_ROWS = 32;          // tokens per block per step (4 waves x 8 rows)
constexpr int QB_MAX_BLOCKS = 1024;  // 4 blocks / CU over all heads; bounds the partials

static inline int qb_grid_x(long M, long heads) {
  return (int)std::max<long>(1, std::min<long>((M + QB_ROWS - 1) / QB_ROWS, QB_MAX_BLOCKS / heads));
}

// qkv: [M, ld], ld = gridDim.y * 128; heads [0, n_rot) are rotated after the bias, the others only biased
__global__ __launch_bounds__(256) void qkv_bias_rope_fwd_kernel(u16* __restrict__ qkv, const u16* __restrict__ bias,
                                                                const float* __restrict__ cosb,
                                                                const float* __restrict__ sinb, int M, int ld,
                                                                int n_rot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (lane & 7) * 8;
  const int col = blockIdx.y * QB_D + p;
  const bool rot = (int)blockIdx.y < n_rot;
  float b1[8], b2[8];
  unpack8(*(const uint4*)(bias + col), b1);
  unpack8(*(const uint4*)(bias + col + 64), b2);
  for (int m = blockIdx.x * QB_ROWS + wave * 8 + (lane >> 3); m < M; m += gridDim.x * QB_ROWS) {
    u16* row = qkv + (long)m * ld + col;
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(*(const uint4*)row, x1);
    unpack8(*(const uint4*)(row + 64), x2);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o1[i] = x1[i] + b1[i];
      o2[i] = x2[i] + b2[i];
    }
    if (rot) {
      float c[8], s[8];
      load8f(cosb + (long)m * 64 + p, c);
      load8f(sinb + (long)m * 64 + p, s);
      rotate_half_fwd(o1, o2, c, s, o1, o2);
    }
    *(uint4*)row = pack8(o1);
    *(uint4*)(row + 64) = pack8(o2);
  }
}

// dqkv: gradient w.r.t. the node's output (in place -> gradient w.r.t. its input: the q|k columns un-rotated, the v
// columns as they are); part: [gridDim.x, ld] fp32, row b = this block's column sums of the un-rotated gradient
__global__ __launch_bounds__(256) void qkv_bias_rope_bwd_kernel(u16* __restrict__ dqkv, const float* __restrict__ cosb,
                                                                const float* __restrict__ sinb,
                                                                float* __restrict__ part, int M, int ld, int n_rot) {
  __shared__ float red[4][QB_D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (lane & 7) * 8;
  const int col = blockIdx.y * QB_D + p;
  const bool rot = (int)blockIdx.y < n_rot;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int m = blockIdx.x * QB_ROWS + wave * 8 + (lane >> 3); m < M; m += gridDim.x * QB_ROWS) {
    u16* row = dqkv + (long)m * ld + col;
    float g[16];
    unpack8(*(const uint4*)row, g);
    unpack8(*(const uint4*)(row + 64), g + 8);
    if (rot) {
      float c[8], s[8];
      load8f(cosb + (long)m * 64 + p, c);
      load8f(sinb + (long)m * 64 + p, s);
      rotate_half_inv(g, g + 8, c, s, g, g + 8);
      *(uint4*)row = pack8(g);
      *(uint4*)(row + 64) = pack8(g + 8);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += g[i];
  }
  // every lane is back here. This is wave_colsum128 (qkv_rows.h) written out: behind a call the compiler splits the
  // block after this kernel's divergent token loop and schedules it differently (profiles/shared_kernel_headers.md)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) acc[i] += __shfl_xor(acc[i], o, 64);
  }
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[wave][p + i] = acc[i];
      red[wave][64 + p + i] = acc[8 + i];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < QB_D)
    part[(long)blockIdx.x * ld + blockIdx.y * QB_D + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// out[c] = part[0, c] + part[1, c] + ... in that order (rows <= 341), one column per thread, four loads in flight
__global__ __launch_bounds__(256) void qkv_bias_dbias_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                             int rows, int ld) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ld) return;
  float acc = 0.f;
  int b = 0;
  for (; b + 4 <= rows; b += 4) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = part[(long)(b + k) * ld + c];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += v[k];
  }
  for (; b < rows; ++b) acc += part[(long)b * ld + c];
  out[c] = acc;
}

static long qb_check(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin, int64_t n_q, int64_t n_kv,
                     int64_t head_dim) {
  SFT_CHECK(head_dim == QB_D, "qkv_bias_rope: head_dim must be 128");
  SFT_CHECK(n_q > 0 && n_kv > 0 && n_q + 2 * n_kv <= QB_MAX_BLOCKS, "qkv_bias_rope: head counts");
  const long M = check_qkv_rows("qkv_bias_rope", qkv, cos, sin, n_q, n_kv, head_dim, true);
  SFT_CHECK(M < (1L << 31) - (long)QB_MAX_BLOCKS * QB_ROWS, "qkv_bias_rope: too many rows for 32-bit indexing");
  return M;
}

void qkv_bias_rope_fwd(at::Tensor qkv, const at::Tensor& bias, const at::Tensor& cos, const at::Tensor& sin,
                       int64_t n_q, int64_t n_kv, int64_t head_dim) {
  const long M = qb_check(qkv, cos, sin, n_q, n_kv, head_dim);
  const int heads = n_q + 2 * n_kv;
  SFT_CHECK_BF16(bias);
  SFT_CHECK(bias.is_cuda() && bias.is_contiguous() && bias.numel() == (long)heads * QB_D &&
                ((uintptr_t)bias.data_ptr() & 15) == 0,
            "qkv_bias_rope: bias must be contiguous bf16 [(n_q + 2 n_kv) * 128] on the GPU, 16-byte aligned");
  if (M == 0) return;
  SFT_TRACE("ew.qkv_bias_rope.fwd");
  qkv_bias_rope_fwd_kernel<<<dim3(qb_grid_x(M, heads), heads), 256, 0, cur_stream()>>>(
      (u16*)qkv.data_ptr(), (const u16*)bias.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), (int)M,
      heads * QB_D, (int)(n_q + n_kv));
  SFT_LAUNCH_CHECK();
}

at::Tensor qkv_bias_rope_bwd(at::Tensor dqkv, const at::Tensor& cos, const at::Tensor& sin, int64_t n_q, int64_t n_kv,
                             int64_t head_dim) {
  const long M = qb_check(dqkv, cos, sin, n_q, n_kv, head_dim);
  const int heads = n_q + 2 * n_kv, ld = heads * QB_D;
  auto fopt = dqkv.options().dtype(at::kFloat);
  if (M == 0) return at::zeros({ld}, fopt);
  auto dbias = at::empty({ld}, fopt);
  const int gx = qb_grid_x(M, heads);
  auto part = at::empty({gx, ld}, fopt);
  SFT_TRACE("ew.qkv_bias_rope.bwd");
  qkv_bias_rope_bwd_kernel<<<dim3(gx, heads), 256, 0, cur_stream()>>>((u16*)dqkv.data_ptr(), cos.data_ptr<float>(),
                                                                       sin.data_ptr<float>(), part.data_ptr<float>(),
                                                                       (int)M, ld, (int)(n_q + n_kv));
  SFT_LAUNCH_CHECK();
  qkv_bias_dbias_kernel<<<(ld + 255) / 256, 256, 0, cur_stream()>>>(part.data_ptr<float>(), dbias.data_ptr<float>(),
                                                                    gx, ld);
  SFT_LAUNCH_CHECK();
  return dbias;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("qkv_bias_rope_fwd", &qkv_bias_rope_fwd);
  m.impl("qkv_bias_rope_bwd", &qkv_bias_rope_bwd);
}

}  // namespace sftamd
