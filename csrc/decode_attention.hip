// Single-token GQA decode attention over a preallocated KV cache (inference).
//
// Split-K ("flash-decoding"): grid (splits, kv_heads); each 256-thread workgroup scores one
// 256-key chunk for ALL query heads of its GQA group (K/V rows are read once per group, 16-byte
// loads), keeps the chunk's (max, sum, unnormalised P.V) in fp32, and a combine kernel merges
// the splits. The live cache length is read from DEVICE memory, so the whole decode step has
// static shapes and is captured once into a hipGraph and replayed per token (no host sync,
// no per-layer launch overhead).
//
// decode_attention_batched runs the same step for B sequences at once: grid (splits, kv_heads, B), each block
// reading its own sequence's length, after an append kernel has stored the step's K/V rows in the caches.
#include "common.h"

namespace sftamd {
namespace decode {

constexpr int D = 128;
constexpr int CHUNK = 256;
constexpr int MAXREP = 8;
constexpr float LOG2E = 1.4426950408889634f;

// One (split, kv head) workgroup of one sequence; shared by the single-sequence and the batched kernel.
// q: [nq*D] bf16; kc/vc: [S_max, nkv, D] bf16; po: [rep, D] f32; pml: [rep, 2] f32 (this block's partials)
// window > 0 (sliding window): the live keys are [max(0, len - window), len); a chunk wholly below them is empty,
// the chunk that straddles the edge masks its low keys.
__device__ __forceinline__ void split_body(const u16* __restrict__ q, const u16* __restrict__ kc,
                                           const u16* __restrict__ vc, const int len, float* __restrict__ po,
                                           float* __restrict__ pml, const int split, const int kvh, int nq, int nkv,
                                           float sl2, int window) {
  __shared__ float qs[MAXREP][D];
  __shared__ float ps[MAXREP][CHUNK];
  __shared__ float red[MAXREP][8];
  __shared__ float acc2[2][MAXREP][D];
  const int rep = nq / nkv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = split * CHUNK;
  const int lo = window > 0 ? max(len - window, 0) : 0;  // first live key
  if (k0 >= len || k0 + CHUNK <= lo) {  // empty chunk: neutral element for the combine
    if (tid < rep) {
      pml[tid * 2] = -INFINITY;
      pml[tid * 2 + 1] = 0.f;
    }
    return;
  }
  for (int i = tid; i < rep * D; i += 256) qs[i / D][i % D] = bf2f(q[(long)(kvh * rep + i / D) * D + i % D]);
  __syncthreads();
  const int key = k0 + tid;
  float s[MAXREP];
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) s[h] = -INFINITY;
  const bool live = key < len && key >= lo;
  if (live) {
    const u16* kr = kc + ((long)key * nkv + kvh) * D;
#pragma unroll
    for (int h = 0; h < MAXREP; ++h) s[h] = 0.f;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
      float kf[8];
      unpack8(*(const uint4*)(kr + c * 8), kf);
#pragma unroll
      for (int h = 0; h < MAXREP; ++h)
        if (h < rep) {
#pragma unroll
          for (int e = 0; e < 8; ++e) s[h] += kf[e] * qs[h][c * 8 + e];
        }
    }
#pragma unroll
    for (int h = 0; h < MAXREP; ++h) s[h] *= sl2;
  }
  // chunk max / sum per head
  float m[MAXREP], l[MAXREP];
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) {
    float v = wave_max(s[h]);
    if (lane == 0) red[h][wave] = v;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) m[h] = fmaxf(fmaxf(red[h][0], red[h][1]), fmaxf(red[h][2], red[h][3]));
  __syncthreads();
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) {
    const float p = (h < rep && live) ? exp2f(s[h] - m[h]) : 0.f;
    if (h < rep) ps[h][tid] = p;
    const float v = wave_sum(p);
    if (lane == 0) red[h][4 + wave] = v;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) l[h] = (red[h][4] + red[h][5]) + (red[h][6] + red[h][7]);
  // P.V: thread -> (dim d, key parity kh)
  const int d = tid & (D - 1), kh = tid >> 7;
  float a[MAXREP];
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) a[h] = 0.f;
  const int nk = min(CHUNK, len - k0);
  for (int t = max(lo - k0, 0) + kh; t < nk; t += 2) {
    const float v = bf2f(vc[((long)(k0 + t) * nkv + kvh) * D + d]);
#pragma unroll
    for (int h = 0; h < MAXREP; ++h)
      if (h < rep) a[h] += ps[h][t] * v;
  }
#pragma unroll
  for (int h = 0; h < MAXREP; ++h)
    if (h < rep) acc2[kh][h][d] = a[h];
  __syncthreads();
  if (kh == 0) {
    for (int h = 0; h < rep; ++h) po[h * D + d] = acc2[0][h][d] + acc2[1][h][d];
  }
  if (tid < rep) {
    pml[tid * 2] = m[tid];
    pml[tid * 2 + 1] = l[tid];
  }
}

// part_o: [nkv, splits, rep, D] f32; part_ml: [nkv, splits, rep, 2]
__global__ __launch_bounds__(256) void split_kernel(const u16* __restrict__ q, const u16* __restrict__ kc,
                                                    const u16* __restrict__ vc, const int* __restrict__ len_p,
                                                    float* __restrict__ part_o, float* __restrict__ part_ml, int nq,
                                                    int nkv, float sl2, int window) {
  const int split = blockIdx.x, kvh = blockIdx.y, splits = gridDim.x;
  const int rep = nq / nkv;
  split_body(q, kc, vc, *len_p, part_o + ((long)(kvh * splits + split) * rep) * D,
             part_ml + ((long)(kvh * splits + split) * rep) * 2, split, kvh, nq, nkv, sl2, window);
}

// Merge of one query head's splits. EMPTY_OK: a sequence with no live key (every chunk empty) gives zeros, not 0/0.
template <bool EMPTY_OK>
__device__ __forceinline__ void combine_body(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                             u16* __restrict__ out, const int hq, int nq, int nkv, int splits) {
  const int d = threadIdx.x;
  const int rep = nq / nkv, kvh = hq / rep, h = hq - kvh * rep;
  float M = -INFINITY;
  for (int s = 0; s < splits; ++s) M = fmaxf(M, part_ml[((long)(kvh * splits + s) * rep + h) * 2]);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < splits; ++s) {
    const long b = (long)(kvh * splits + s) * rep + h;
    const float ms = part_ml[b * 2];
    if (ms == -INFINITY) continue;
    const float w = exp2f(ms - M);
    L += w * part_ml[b * 2 + 1];
    O += w * part_o[b * D + d];
  }
  if (EMPTY_OK && L == 0.f) {
    out[(long)hq * D + d] = 0;
    return;
  }
  out[(long)hq * D + d] = f2bf(O / L);
}

__global__ __launch_bounds__(128) void combine_kernel(const float* __restrict__ part_o,
                                                      const float* __restrict__ part_ml, u16* __restrict__ out,
                                                      int nq, int nkv, int splits) {
  combine_body<false>(part_o, part_ml, out, blockIdx.x, nq, nkv, splits);
}

// ---- batched decode: B sequences, one slab [S_max, nkv, D] each, one step's packed qkv row each -----------------

// Row b's K and V of this step -> cache[b, lens[b] - 1]. One block per sequence, 16-byte loads and stores.
// A length outside (0, S_max] skips the row: a host bug must not become an out-of-bounds write.
__global__ __launch_bounds__(256) void append_kernel(const u16* __restrict__ qkv, u16* __restrict__ kc,
                                                     u16* __restrict__ vc, const int* __restrict__ lens, int nq,
                                                     int nkv, int smax) {
  const int b = blockIdx.x;
  const int len = lens[b];
  if (len <= 0 || len > smax) return;
  const int nvec = nkv * D / 8;  // uint4 per K (and per V) row
  const uint4* src = (const uint4*)(qkv + (long)b * (nq + 2 * nkv) * D + (long)nq * D);
  const long row = ((long)b * smax + (len - 1)) * nvec;
  uint4* kd = (uint4*)kc + row;
  uint4* vd = (uint4*)vc + row;
  for (int i = threadIdx.x; i < nvec; i += 256) {
    kd[i] = src[i];
    vd[i] = src[nvec + i];
  }
}

// grid (splits, nkv, B). qkv: [B, (nq + 2 nkv) * D]; kc/vc: [B, S_max, nkv, D]; part_o: [B, nkv, splits, rep, D]
__global__ __launch_bounds__(256) void split_batched_kernel(const u16* __restrict__ qkv, const u16* __restrict__ kc,
                                                            const u16* __restrict__ vc, const int* __restrict__ lens,
                                                            float* __restrict__ part_o, float* __restrict__ part_ml,
                                                            int nq, int nkv, int smax, float sl2, int window) {
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, splits = gridDim.x;
  const int rep = nq / nkv;
  const int len = min(lens[b], smax);  // never read past the slab; <= 0 leaves every chunk empty
  const long blk = ((long)b * nkv + kvh) * splits + split;
  const long slab = (long)b * smax * nkv * D;
  split_body(qkv + (long)b * (nq + 2 * nkv) * D, kc + slab, vc + slab, len, part_o + blk * rep * D,
             part_ml + blk * rep * 2, split, kvh, nq, nkv, sl2, window);
}

// grid (nq, B)
__global__ __launch_bounds__(128) void combine_batched_kernel(const float* __restrict__ part_o,
                                                              const float* __restrict__ part_ml,
                                                              u16* __restrict__ out, int nq, int nkv, int splits) {
  const int b = blockIdx.y;
  combine_body<true>(part_o + (long)b * nq * splits * D, part_ml + (long)b * nq * splits * 2,
                     out + (long)b * nq * D, blockIdx.x, nq, nkv, splits);
}

}  // namespace decode

at::Tensor decode_attention(const at::Tensor& q, const at::Tensor& kcache, const at::Tensor& vcache,
                            const at::Tensor& cache_len, int64_t nq, int64_t nkv, double scale, int64_t window) {
  SFT_CHECK_BF16(q);
  SFT_CHECK_BF16(kcache);
  SFT_CHECK(q.is_contiguous() && kcache.is_contiguous() && vcache.is_contiguous(), "contiguous");
  SFT_CHECK(kcache.dim() == 3 && kcache.size(1) == nkv && kcache.size(2) == decode::D, "kcache [S, nkv, 128]");
  SFT_CHECK(q.numel() == nq * decode::D, "q must be [nq*128]");
  SFT_CHECK(nq % nkv == 0 && nq / nkv <= decode::MAXREP, "GQA ratio <= 8");
  SFT_CHECK(cache_len.scalar_type() == at::kInt && cache_len.is_cuda(), "cache_len int32 on device");
  SFT_CHECK(window >= 0, "decode_attention: window must be >= 0");
  const int smax = kcache.size(0);
  const int win = window < smax ? (int)window : 0;  // a window that covers the cache is no window
  const int splits = (smax + decode::CHUNK - 1) / decode::CHUNK;
  const int rep = nq / nkv;
  auto po = at::empty({nkv * splits * rep * decode::D}, q.options().dtype(at::kFloat));
  auto pml = at::empty({nkv * splits * rep * 2}, q.options().dtype(at::kFloat));
  auto out = at::empty({nq * decode::D}, q.options());
  decode::split_kernel<<<dim3(splits, nkv), 256, 0, cur_stream()>>>(
      (const u16*)q.data_ptr(), (const u16*)kcache.data_ptr(), (const u16*)vcache.data_ptr(), cache_len.data_ptr<int>(),
      po.data_ptr<float>(), pml.data_ptr<float>(), nq, nkv, (float)scale * decode::LOG2E, win);
  SFT_LAUNCH_CHECK();
  decode::combine_kernel<<<nq, 128, 0, cur_stream()>>>(po.data_ptr<float>(), pml.data_ptr<float>(),
                                                       (u16*)out.data_ptr(), nq, nkv, splits);
  SFT_LAUNCH_CHECK();
  return out;
}

// One decode step of B sequences: append row b's K/V at cache[b, lens[b] - 1], then attend over cache[b, :lens[b]].
// qkv [B, (nq + 2 nkv) * 128] (post-RoPE), kcache / vcache [B, S_max, nkv, 128], lens int32 [B] on the device
// (live length INCLUDING the token being decoded). Static shapes, no host sync: lives inside a captured graph.
at::Tensor decode_attention_batched(const at::Tensor& qkv, at::Tensor kcache, at::Tensor vcache, const at::Tensor& lens,
                                    int64_t nq, int64_t nkv, double scale, int64_t window) {
  SFT_CHECK_CUDA(qkv);
  SFT_CHECK_BF16(qkv);
  SFT_CHECK_BF16(kcache);
  SFT_CHECK_BF16(vcache);
  SFT_CHECK(qkv.is_contiguous() && kcache.is_contiguous() && vcache.is_contiguous(), "contiguous");
  SFT_CHECK(nq > 0 && nkv > 0 && nq % nkv == 0 && nq / nkv <= decode::MAXREP, "GQA ratio <= 8");
  SFT_CHECK(qkv.dim() == 2 && qkv.size(1) == (nq + 2 * nkv) * decode::D, "qkv must be [B, (nq + 2 nkv) * 128]");
  const int64_t B = qkv.size(0);
  SFT_CHECK(kcache.dim() == 4 && kcache.size(0) == B && kcache.size(2) == nkv && kcache.size(3) == decode::D,
            "kcache [B, S, nkv, 128]");
  SFT_CHECK(vcache.sizes() == kcache.sizes() && kcache.is_cuda() && vcache.is_cuda(), "vcache must match kcache");
  SFT_CHECK(lens.scalar_type() == at::kInt && lens.is_cuda() && lens.is_contiguous() && lens.numel() == B,
            "lens int32 [B] on device");
  SFT_CHECK(B >= 1 && B <= 65535, "batch size");
  SFT_CHECK((uintptr_t)qkv.data_ptr() % 16 == 0 && (uintptr_t)kcache.data_ptr() % 16 == 0 &&
                (uintptr_t)vcache.data_ptr() % 16 == 0, "16-byte aligned");
  const int smax = kcache.size(1);
  SFT_CHECK(smax >= 1, "empty cache");
  SFT_CHECK(window >= 0, "decode_attention_batched: window must be >= 0");
  const int win = window < smax ? (int)window : 0;  // a window that covers the slab is no window
  const int splits = (smax + decode::CHUNK - 1) / decode::CHUNK;
  const int rep = nq / nkv;
  auto po = at::empty({B * nkv * splits * rep * decode::D}, qkv.options().dtype(at::kFloat));
  auto pml = at::empty({B * nkv * splits * rep * 2}, qkv.options().dtype(at::kFloat));
  auto out = at::empty({B, nq * decode::D}, qkv.options());
  decode::append_kernel<<<B, 256, 0, cur_stream()>>>((const u16*)qkv.data_ptr(), (u16*)kcache.data_ptr(),
                                                     (u16*)vcache.data_ptr(), lens.data_ptr<int>(), nq, nkv, smax);
  SFT_LAUNCH_CHECK();
  decode::split_batched_kernel<<<dim3(splits, nkv, B), 256, 0, cur_stream()>>>(
      (const u16*)qkv.data_ptr(), (const u16*)kcache.data_ptr(), (const u16*)vcache.data_ptr(), lens.data_ptr<int>(),
      po.data_ptr<float>(), pml.data_ptr<float>(), nq, nkv, smax, (float)scale * decode::LOG2E, win);
  SFT_LAUNCH_CHECK();
  decode::combine_batched_kernel<<<dim3(nq, B), 128, 0, cur_stream()>>>(po.data_ptr<float>(), pml.data_ptr<float>(),
                                                                        (u16*)out.data_ptr(), nq, nkv, splits);
  SFT_LAUNCH_CHECK();
  return out;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("decode_attention", &decode_attention);
  m.impl("decode_attention_batched", &decode_attention_batched);
}

}  // namespace sftamd
