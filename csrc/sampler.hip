// Fused decode-time sampler for gfx950: repetition penalty -> temperature -> top-k ->
// top-p -> multinomial draw, for one sequence over the full vocabulary, with no host round trip.
//
// The reference's generate() (ask_tuned_model.py:55-65 via HF) runs this as a chain of ~15 eager
// kernels plus a host sync per token (multinomial + .item()). Here it is two launches that can live
// inside the hipGraph of the decode step:
//   partial: grid of 2048-logit tiles, one 256-thread block each; logits read once (bf16 or fp32),
//            penalty from a device presence bitmask (the generated history as a set), scaled by
//            1/temperature, block radix sort (rocPRIM, 8 keys/thread), top K candidates written out;
//   final:   one block merges the <= 4096 candidates (radix sort, 16 keys/thread), then one wave-lane
//            applies softmax over the top K, the top-p cut (a token is dropped once the probability
//            mass ranked above it exceeds top_p — the same rule as inference/generation.py
//            sample_next) and draws with a counter-based uniform (hash of seed and the device step
//            counter, so every graph replay draws fresh). It writes the token to the next step's
//            embedding input, to a device token log, sets the token's presence bit and advances the
//            counters (position, KV length, step) — the decode loop runs replay after replay.
// sample_tokens is the same pair of launches for B rows (grid (tiles, B), then one merge block per row) with a
// per-row finished flag: batched generation decodes many prompts per step.
#include "common.h"

#include <rocprim/block/block_radix_sort.hpp>

namespace sftamd {
namespace samp {

constexpr int NT = 256;
constexpr int IPT = 8;                  // keys per thread, partial pass
constexpr int TILE = NT * IPT;          // 2048 logits per block
constexpr int IPT2 = 16;                // keys per thread, final pass (4096 candidates)
constexpr int KMAX = 64;                // top-k supported on the device path

// IPT consecutive logits i0 .. i0 + IPT - 1 of a row as floats (elements at or past V are left unset): 16-byte vector
// loads when the run is whole and aligned (a row of a [B, V] batch with odd V is not), element loads otherwise.
template <typename T>
__device__ __forceinline__ void load_run(const T* __restrict__ logits, int i0, int V, float* raw);
template <>
__device__ __forceinline__ void load_run<float>(const float* __restrict__ logits, int i0, int V, float* raw) {
  const float* p = logits + i0;
  if (i0 + IPT <= V && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *(float4*)&raw[0] = *(const float4*)p;
    *(float4*)&raw[4] = *(const float4*)(p + 4);
  } else {
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      if (i0 + j < V) raw[j] = p[j];
  }
}
template <>
__device__ __forceinline__ void load_run<u16>(const u16* __restrict__ logits, int i0, int V, float* raw) {
  const u16* p = logits + i0;
  if (i0 + IPT <= V && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    unpack8(*(const uint4*)p, raw);
  } else {
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      if (i0 + j < V) raw[j] = bf2f(p[j]);
  }
}

// One 2048-logit tile of one row (shared by the single-row and the batched kernel): logits / presence / cand_* point
// at the row, ``tile`` is the tile's index within it.
template <typename T>
__device__ __forceinline__ void partial_body(const T* __restrict__ logits, int V,
                                             const unsigned* __restrict__ presence, float inv_temp, float penalty,
                                             int K, float* __restrict__ cand_v, int* __restrict__ cand_i,
                                             const int tile) {
  using Sort = rocprim::block_radix_sort<float, NT, IPT, int>;
  __shared__ typename Sort::storage_type storage;
  float key[IPT];
  int idx[IPT];
  // Blocked loads: thread t holds logits i0 .. i0 + IPT - 1 in index order. The radix sort is stable and its input
  // order is (thread, j), so equal keys keep their index order and a tie at the top resolves to the LOWEST index, as
  // argmax does on the host path (striped loads resolved a tie between indices 1 and 256 of a tile to 256).
  const int i0 = tile * TILE + threadIdx.x * IPT;
  float raw[IPT];
  load_run<T>(logits, i0, V, raw);
  // i0 is a multiple of IPT = 8: the 8 presence bits of the run sit in one word
  const unsigned pres = (penalty != 1.f && i0 < V) ? (presence[i0 >> 5] >> (i0 & 31)) & 0xffu : 0u;
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int i = i0 + j;
    float x = -INFINITY;
    if (i < V) {
      x = raw[j];
      if ((pres >> j) & 1u) x = x < 0.f ? x * penalty : x / penalty;
      x *= inv_temp;
    }
    key[j] = x;
    idx[j] = i < V ? i : 0x7fffffff;
  }
  Sort().sort_desc(key, idx, storage);  // blocked result: thread t holds ranks IPT t .. IPT t + IPT - 1
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int r = threadIdx.x * IPT + j;
    if (r < K) {
      cand_v[tile * K + r] = key[j];
      cand_i[tile * K + r] = idx[j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void partial_kernel(const T* __restrict__ logits, int V,
                                                     const unsigned* __restrict__ presence, float inv_temp,
                                                     float penalty, int K, float* __restrict__ cand_v,
                                                     int* __restrict__ cand_i) {
  partial_body<T>(logits, V, presence, inv_temp, penalty, K, cand_v, cand_i, blockIdx.x);
}

// grid (tiles, B): logits [B, V], presence [B, words], cand_* [B, tiles * K]. A finished row is skipped.
template <typename T>
__global__ __launch_bounds__(NT) void partial_batched_kernel(const T* __restrict__ logits, int V,
                                                             const unsigned* __restrict__ presence, int words,
                                                             float inv_temp, float penalty, int K,
                                                             float* __restrict__ cand_v, int* __restrict__ cand_i,
                                                             const int* __restrict__ done) {
  const int b = blockIdx.y;
  if (done[b]) return;
  const long nc = (long)gridDim.x * K;
  partial_body<T>(logits + (long)b * V, V, presence + (long)b * words, inv_temp, penalty, K, cand_v + b * nc,
                  cand_i + b * nc, blockIdx.x);
}

// The merge + draw of one row (shared by the single-row and the batched kernel); every pointer is the row's own.
// ``done`` (batched only, else null) is the row's finished flag: drawing ``eos`` logs the token, sets the flag and
// leaves position / KV length where they are (the EOS is never decoded).
// state (int64): [0] step counter (RNG), [1] last token, [2] position, [3] KV length (int64 mirror)
__device__ __forceinline__ void final_body(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                           int ncand, int K, float top_p, int do_sample, unsigned seed,
                                           long long* __restrict__ state, long long* __restrict__ tok_out,
                                           long long* __restrict__ pos_out, int* __restrict__ len_out,
                                           long long* __restrict__ log, int log_cap, unsigned* __restrict__ presence,
                                           int* __restrict__ done, int eos) {
  using Sort = rocprim::block_radix_sort<float, NT, IPT2, int>;
  __shared__ typename Sort::storage_type storage;
  __shared__ float top_v[KMAX];
  __shared__ int top_i[KMAX];
  float key[IPT2];
  int idx[IPT2];
#pragma unroll
  for (int j = 0; j < IPT2; ++j) {
    const int c = threadIdx.x * IPT2 + j;  // blocked: candidates are (tile, rank)-ordered, so ties keep index order
    key[j] = c < ncand ? cand_v[c] : -INFINITY;
    idx[j] = c < ncand ? cand_i[c] : 0x7fffffff;
  }
  Sort().sort_desc(key, idx, storage);
#pragma unroll
  for (int j = 0; j < IPT2; ++j) {
    const int r = threadIdx.x * IPT2 + j;
    if (r < K) {
      top_v[r] = key[j];
      top_i[r] = idx[j];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long step = state[0];
  int tok = top_i[0];
  if (do_sample) {
    const float m = top_v[0];
    float z = 0.f;
    for (int r = 0; r < K; ++r) z += __expf(top_v[r] - m);
    // top-p: keep rank r while the mass ranked above it is <= top_p (rank 0 always kept)
    float above = 0.f, kept = 0.f;
    int n = 0;
    for (; n < K; ++n) {
      if (n > 0 && above > top_p) break;
      const float p = __expf(top_v[n] - m) / z;
      above += p;
      kept += p;
    }
    const unsigned h = hash_u32((unsigned long long)step, seed);
    const float u = ((h >> 8) + 0.5f) * (1.f / 16777216.f) * kept;  // uniform in (0, kept)
    float c = 0.f;
    tok = top_i[n - 1];
    for (int r = 0; r < n; ++r) {
      c += __expf(top_v[r] - m) / z;
      if (u <= c) {
        tok = top_i[r];
        break;
      }
    }
  }
  state[0] = step + 1;
  state[1] = tok;
  if (tok_out) tok_out[0] = tok;
  if (log && step < log_cap) log[step] = tok;
  const bool finished = done != nullptr && tok == eos;
  if (finished) *done = 1;
  if (pos_out && !finished) {  // advance the decode step's position / KV length for the next replay
    const long long p = state[2] + 1;
    state[2] = p;
    pos_out[0] = p;
    state[3] = p + 1;
    len_out[0] = (int)(p + 1);
  }
  atomicOr(presence + (tok >> 5), 1u << (tok & 31));
}

__global__ __launch_bounds__(NT) void final_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                   int ncand, int K, float top_p, int do_sample, unsigned seed,
                                                   long long* __restrict__ state, long long* __restrict__ tok_out,
                                                   long long* __restrict__ pos_out, int* __restrict__ len_out,
                                                   long long* __restrict__ log, int log_cap,
                                                   unsigned* __restrict__ presence) {
  final_body(cand_v, cand_i, ncand, K, top_p, do_sample, seed, state, tok_out, pos_out, len_out, log, log_cap,
             presence, nullptr, -1);
}

// One block per row; row b draws with seed + b. A finished row writes nothing at all.
__global__ __launch_bounds__(NT) void final_batched_kernel(const float* __restrict__ cand_v,
                                                           const int* __restrict__ cand_i, int ncand, int K,
                                                           float top_p, int do_sample, unsigned seed,
                                                           long long* __restrict__ state,
                                                           long long* __restrict__ tok_out,
                                                           long long* __restrict__ pos_out, int* __restrict__ len_out,
                                                           long long* __restrict__ log, int log_cap,
                                                           unsigned* __restrict__ presence, int words,
                                                           int* __restrict__ done, int eos) {
  const int b = blockIdx.x;
  if (done[b]) return;
  final_body(cand_v + (long)b * ncand, cand_i + (long)b * ncand, ncand, K, top_p, do_sample, seed + (unsigned)b,
             state + b * 4, tok_out ? tok_out + b : nullptr, pos_out ? pos_out + b : nullptr,
             len_out ? len_out + b : nullptr, log ? log + (long)b * log_cap : nullptr, log_cap,
             presence + (long)b * words, done + b, eos);
}

// ---- the full-vocabulary draw (sample_tokens_full): Gumbel-max. Token i of row b gets the key z_i + g_i with
// z = penalised logit / temperature and g_i = -log(-log u_i), u_i a counter-based uniform of (step, seed + b, i): the
// argmax of the keys is a draw from softmax(z) over the whole vocabulary, with no sort and no cumulative sum. u has 23
// random bits, u = (k + 0.5) 2^-23 (exact in fp32, never 0 or 1), so g lies in [-2.9, 16.7]: a token more than ~19.5
// below the row's best key cannot win, i.e. probabilities below ~e^-16 are cut, far under a bf16 logit's resolution.
// Ties (equal keys) go to the lowest index. The same pass keeps (max z, sum exp(z - max)) for the log-probability
// z_tok - lse(z) of the drawn token.
struct FullAcc {
  float key, z;  // best key and its z
  int idx;       // its index (lowest on a tie)
  float m, s;    // running max z, sum exp(z - m)
};

__device__ __forceinline__ void full_merge(FullAcc& a, const FullAcc& b) {
  if (b.key > a.key || (b.key == a.key && b.idx < a.idx)) {
    a.key = b.key;
    a.z = b.z;
    a.idx = b.idx;
  }
  const float M = fmaxf(a.m, b.m);
  const float ea = (a.m == -INFINITY) ? 0.f : __expf(a.m - M);
  const float eb = (b.m == -INFINITY) ? 0.f : __expf(b.m - M);
  a.s = a.s * ea + b.s * eb;
  a.m = M;
}

// Block-wide full_merge in a fixed order (xor butterfly per wave, then waves 0..3 in order); the result is in thread 0.
__device__ __forceinline__ void full_block_reduce(FullAcc& acc) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    FullAcc b;
    b.key = __shfl_xor(acc.key, o, 64);
    b.z = __shfl_xor(acc.z, o, 64);
    b.idx = __shfl_xor(acc.idx, o, 64);
    b.m = __shfl_xor(acc.m, o, 64);
    b.s = __shfl_xor(acc.s, o, 64);
    full_merge(acc, b);
  }
  __shared__ FullAcc red[NT / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = red[0];
    for (int w = 1; w < NT / 64; ++w) full_merge(acc, red[w]);
  }
}

// grid (tiles, B): one 2048-logit tile of one row; part [B, tiles, 4] = (key, z, max, sum), part_i [B, tiles] = index.
template <typename T>
__global__ __launch_bounds__(NT) void full_partial_kernel(const T* __restrict__ logits, int V,
                                                          const unsigned* __restrict__ presence, int words,
                                                          float inv_temp, float penalty, unsigned seed,
                                                          const long long* __restrict__ state,
                                                          float* __restrict__ part, int* __restrict__ part_i,
                                                          const int* __restrict__ done) {
  const int b = blockIdx.y;
  if (done[b]) return;
  const T* row = logits + (long)b * V;
  const unsigned* pres_row = presence + (long)b * words;
  const unsigned long long step = (unsigned long long)state[(long)b * 4];
  const unsigned sd = seed + (unsigned)b;
  const int i0 = blockIdx.x * TILE + threadIdx.x * IPT;
  float raw[IPT];
  load_run<T>(row, i0, V, raw);
  const unsigned pres = (penalty != 1.f && i0 < V) ? (pres_row[i0 >> 5] >> (i0 & 31)) & 0xffu : 0u;
  FullAcc acc{-INFINITY, -INFINITY, 0x7fffffff, -INFINITY, 0.f};
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int i = i0 + j;
    if (i < V) {
      float x = raw[j];
      if ((pres >> j) & 1u) x = x < 0.f ? x * penalty : x / penalty;
      const float z = x * inv_temp;
      const unsigned h = hash_u32((step << 32) | (unsigned long long)(unsigned)i, sd);
      const float u = ((float)(h >> 9) + 0.5f) * (1.f / 8388608.f);
      const float key = z - logf(0.f - logf(u));
      FullAcc e{key, z, i, z, 1.f};
      full_merge(acc, e);
    }
  }
  full_block_reduce(acc);
  if (threadIdx.x == 0) {
    const long t = (long)b * gridDim.x + blockIdx.x;
    part[t * 4 + 0] = acc.key;
    part[t * 4 + 1] = acc.z;
    part[t * 4 + 2] = acc.m;
    part[t * 4 + 3] = acc.s;
    part_i[t] = acc.idx;
  }
}

// One block per row merges the row's tiles (thread t takes tiles t, t + 256, ... in order), then thread 0 writes what
// final_body writes, plus the log-probability. The row's presence word has this one writer: a plain read-modify-write.
__global__ __launch_bounds__(NT) void full_final_kernel(const float* __restrict__ part, const int* __restrict__ part_i,
                                                        int tiles, int V, long long* __restrict__ state,
                                                        long long* __restrict__ tok_out, long long* __restrict__ pos_out,
                                                        int* __restrict__ len_out, long long* __restrict__ log,
                                                        int log_cap, float* __restrict__ logp_log, int logp_cap,
                                                        unsigned* __restrict__ presence, int words,
                                                        int* __restrict__ done, int eos) {
  const int b = blockIdx.x;
  if (done[b]) return;
  FullAcc acc{-INFINITY, -INFINITY, 0x7fffffff, -INFINITY, 0.f};
  for (int t = threadIdx.x; t < tiles; t += NT) {
    const long q = (long)b * tiles + t;
    FullAcc e{part[q * 4], part[q * 4 + 1], part_i[q], part[q * 4 + 2], part[q * 4 + 3]};
    full_merge(acc, e);
  }
  full_block_reduce(acc);
  if (threadIdx.x != 0) return;
  long long* st = state + (long)b * 4;
  const long long step = st[0];
  int tok = acc.idx;
  if (tok < 0 || tok >= V) tok = 0;  // (a row of NaNs has no best key)
  const float logp = acc.z - (acc.m + __logf(acc.s));
  st[0] = step + 1;
  st[1] = tok;
  if (tok_out) tok_out[b] = tok;
  if (log && step >= 0 && step < log_cap) log[(long)b * log_cap + step] = tok;
  if (step >= 0 && step < logp_cap) logp_log[(long)b * logp_cap + step] = logp;
  const bool finished = tok == eos;
  if (finished) done[b] = 1;
  if (pos_out && !finished) {
    const long long p = st[2] + 1;
    st[2] = p;
    pos_out[b] = p;
    st[3] = p + 1;
    len_out[b] = (int)(p + 1);
  }
  unsigned* pw = presence + (long)b * words + (tok >> 5);
  *pw = *pw | (1u << (tok & 31));
}

}  // namespace samp

// logits [V] (bf16 or fp32). presence int32 bitmask [ceil(V/32)]. state int64 [4]. tok_out / pos_out int64 [1]
// and len_out int32 [1] are optional (the decode graph's inputs). log int64 [cap] optional.
void sample_token(const at::Tensor& logits, at::Tensor presence, at::Tensor state, const c10::optional<at::Tensor>& tok_out,
                  const c10::optional<at::Tensor>& pos_out, const c10::optional<at::Tensor>& len_out,
                  const c10::optional<at::Tensor>& log, double temperature, int64_t top_k, double top_p,
                  double repetition_penalty, bool do_sample, int64_t seed) {
  SFT_CHECK_CUDA(logits);
  SFT_CHECK(logits.is_contiguous() && (logits.scalar_type() == at::kFloat || logits.scalar_type() == at::kBFloat16),
            "sample_token: contiguous fp32/bf16 logits");
  const int V = logits.numel();
  SFT_CHECK(presence.scalar_type() == at::kInt && presence.numel() >= (V + 31) / 32 && presence.is_contiguous(),
            "sample_token: presence int32 bitmask");
  SFT_CHECK(state.scalar_type() == at::kLong && state.numel() >= 4, "sample_token: state int64[4]");
  const int K = do_sample ? (int)top_k : 1;
  SFT_CHECK(K >= 1 && K <= samp::KMAX && K <= V, "sample_token: top_k must be in [1, min(64, V)] on the device path");
  const int nblk = (V + samp::TILE - 1) / samp::TILE;
  SFT_CHECK(nblk * K <= samp::NT * samp::IPT2, "sample_token: vocabulary too large for one merge block");
  SFT_CHECK(!pos_out.has_value() || (len_out.has_value() && pos_out->scalar_type() == at::kLong &&
                                     len_out->scalar_type() == at::kInt), "sample_token: pos int64 / len int32");
  auto cv = at::empty({nblk * K}, logits.options().dtype(at::kFloat));
  auto ci = at::empty({nblk * K}, logits.options().dtype(at::kInt));
  const float inv_t = do_sample ? (float)(1.0 / std::max(temperature, 1e-5)) : 1.f;
  if (logits.scalar_type() == at::kFloat)
    samp::partial_kernel<float><<<nblk, samp::NT, 0, cur_stream()>>>(
        logits.data_ptr<float>(), V, (const unsigned*)presence.data_ptr<int>(), inv_t, (float)repetition_penalty, K,
        cv.data_ptr<float>(), ci.data_ptr<int>());
  else
    samp::partial_kernel<u16><<<nblk, samp::NT, 0, cur_stream()>>>(
        (const u16*)logits.data_ptr(), V, (const unsigned*)presence.data_ptr<int>(), inv_t, (float)repetition_penalty,
        K, cv.data_ptr<float>(), ci.data_ptr<int>());
  SFT_LAUNCH_CHECK();
  samp::final_kernel<<<1, samp::NT, 0, cur_stream()>>>(
      cv.data_ptr<float>(), ci.data_ptr<int>(), nblk * K, K, (float)top_p, do_sample ? 1 : 0, (unsigned)seed,
      (long long*)state.data_ptr<int64_t>(), tok_out.has_value() ? (long long*)tok_out->data_ptr<int64_t>() : nullptr,
      pos_out.has_value() ? (long long*)pos_out->data_ptr<int64_t>() : nullptr,
      len_out.has_value() ? len_out->data_ptr<int>() : nullptr,
      log.has_value() ? (long long*)log->data_ptr<int64_t>() : nullptr, log.has_value() ? (int)log->numel() : 0,
      (unsigned*)presence.data_ptr<int>());
  SFT_LAUNCH_CHECK();
}

// B rows at once: logits [B, V] (bf16 or fp32), presence int32 [B, >= ceil(V/32)], state int64 [B, 4], done int32 [B];
// tok_out / pos_out int64 [B], len_out int32 [B] and log int64 [B, cap] are optional. Row b applies sample_token's
// rules with seed + b, so row 0 reproduces sample_token with the same seed. A row that draws eos_token_id (-1: none)
// logs it and sets done[b]; a row whose done[b] is set is skipped entirely.
void sample_tokens(const at::Tensor& logits, at::Tensor presence, at::Tensor state, const c10::optional<at::Tensor>& tok_out,
                   const c10::optional<at::Tensor>& pos_out, const c10::optional<at::Tensor>& len_out,
                   const c10::optional<at::Tensor>& log, at::Tensor done, int64_t eos_token_id, double temperature,
                   int64_t top_k, double top_p, double repetition_penalty, bool do_sample, int64_t seed) {
  SFT_CHECK_CUDA(logits);
  SFT_CHECK(logits.dim() == 2 && logits.is_contiguous() &&
                (logits.scalar_type() == at::kFloat || logits.scalar_type() == at::kBFloat16),
            "sample_tokens: contiguous fp32/bf16 logits [B, V]");
  const int64_t B = logits.size(0);
  const int V = logits.size(1);
  SFT_CHECK(B >= 1 && B <= 65535 && V >= 1, "sample_tokens: batch size");
  SFT_CHECK(presence.is_cuda() && presence.scalar_type() == at::kInt && presence.dim() == 2 && presence.size(0) == B &&
                presence.size(1) >= (V + 31) / 32 && presence.is_contiguous(),
            "sample_tokens: presence int32 bitmask [B, ceil(V/32)]");
  SFT_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.dim() == 2 && state.size(0) == B &&
                state.size(1) == 4 && state.is_contiguous(), "sample_tokens: state int64 [B, 4]");
  SFT_CHECK(done.is_cuda() && done.scalar_type() == at::kInt && done.numel() == B && done.is_contiguous(),
            "sample_tokens: done int32 [B]");
  const int K = do_sample ? (int)top_k : 1;
  SFT_CHECK(K >= 1 && K <= samp::KMAX && K <= V, "sample_tokens: top_k must be in [1, min(64, V)] on the device path");
  const int nblk = (V + samp::TILE - 1) / samp::TILE;
  SFT_CHECK(nblk * K <= samp::NT * samp::IPT2, "sample_tokens: vocabulary too large for one merge block");
  SFT_CHECK(!tok_out.has_value() || (tok_out->is_cuda() && tok_out->scalar_type() == at::kLong &&
                                     tok_out->numel() == B && tok_out->is_contiguous()), "sample_tokens: tok int64 [B]");
  SFT_CHECK(!pos_out.has_value() ||
                (len_out.has_value() && pos_out->is_cuda() && len_out->is_cuda() && pos_out->scalar_type() == at::kLong &&
                 len_out->scalar_type() == at::kInt && pos_out->numel() == B && len_out->numel() == B &&
                 pos_out->is_contiguous() && len_out->is_contiguous()), "sample_tokens: pos int64 [B] / len int32 [B]");
  SFT_CHECK(!log.has_value() || (log->is_cuda() && log->scalar_type() == at::kLong && log->dim() == 2 &&
                                 log->size(0) == B && log->is_contiguous()), "sample_tokens: log int64 [B, cap]");
  auto cv = at::empty({B * nblk * K}, logits.options().dtype(at::kFloat));
  auto ci = at::empty({B * nblk * K}, logits.options().dtype(at::kInt));
  const float inv_t = do_sample ? (float)(1.0 / std::max(temperature, 1e-5)) : 1.f;
  const int words = presence.size(1);
  if (logits.scalar_type() == at::kFloat)
    samp::partial_batched_kernel<float><<<dim3(nblk, B), samp::NT, 0, cur_stream()>>>(
        logits.data_ptr<float>(), V, (const unsigned*)presence.data_ptr<int>(), words, inv_t,
        (float)repetition_penalty, K, cv.data_ptr<float>(), ci.data_ptr<int>(), done.data_ptr<int>());
  else
    samp::partial_batched_kernel<u16><<<dim3(nblk, B), samp::NT, 0, cur_stream()>>>(
        (const u16*)logits.data_ptr(), V, (const unsigned*)presence.data_ptr<int>(), words, inv_t,
        (float)repetition_penalty, K, cv.data_ptr<float>(), ci.data_ptr<int>(), done.data_ptr<int>());
  SFT_LAUNCH_CHECK();
  samp::final_batched_kernel<<<B, samp::NT, 0, cur_stream()>>>(
      cv.data_ptr<float>(), ci.data_ptr<int>(), nblk * K, K, (float)top_p, do_sample ? 1 : 0, (unsigned)seed,
      (long long*)state.data_ptr<int64_t>(), tok_out.has_value() ? (long long*)tok_out->data_ptr<int64_t>() : nullptr,
      pos_out.has_value() ? (long long*)pos_out->data_ptr<int64_t>() : nullptr,
      len_out.has_value() ? len_out->data_ptr<int>() : nullptr,
      log.has_value() ? (long long*)log->data_ptr<int64_t>() : nullptr, log.has_value() ? (int)log->size(1) : 0,
      (unsigned*)presence.data_ptr<int>(), words, done.data_ptr<int>(), (int)eos_token_id);
  SFT_LAUNCH_CHECK();
}

// sample_tokens' rows, state and outputs with the draw taken from softmax(penalised logits / temperature) over the WHOLE
// vocabulary (no top-k, no top-p): what a policy-gradient ratio needs. logp_log fp32 [B, cap] receives the drawn
// token's log-probability under that distribution at the row's step. The draw depends only on (seed + b, the row's
// step counter, the logits); no atomics, so a repeated call draws the same tokens.
void sample_tokens_full(const at::Tensor& logits, at::Tensor presence, at::Tensor state,
                        const c10::optional<at::Tensor>& tok_out, const c10::optional<at::Tensor>& pos_out,
                        const c10::optional<at::Tensor>& len_out, const c10::optional<at::Tensor>& log,
                        at::Tensor logp_log, at::Tensor done, int64_t eos_token_id, double temperature,
                        double repetition_penalty, int64_t seed) {
  SFT_CHECK_CUDA(logits);
  SFT_CHECK(logits.dim() == 2 && logits.is_contiguous() &&
                (logits.scalar_type() == at::kFloat || logits.scalar_type() == at::kBFloat16),
            "sample_tokens_full: contiguous fp32/bf16 logits [B, V]");
  const int64_t B = logits.size(0);
  SFT_CHECK(B >= 1 && B <= 65535 && logits.size(1) >= 1 && logits.size(1) < (1L << 31) - samp::TILE,
            "sample_tokens_full: batch size / vocabulary");
  const int V = logits.size(1);
  SFT_CHECK(presence.is_cuda() && presence.scalar_type() == at::kInt && presence.dim() == 2 && presence.size(0) == B &&
                presence.size(1) >= (V + 31) / 32 && presence.is_contiguous(),
            "sample_tokens_full: presence int32 bitmask [B, ceil(V/32)]");
  SFT_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.dim() == 2 && state.size(0) == B &&
                state.size(1) == 4 && state.is_contiguous(), "sample_tokens_full: state int64 [B, 4]");
  SFT_CHECK(done.is_cuda() && done.scalar_type() == at::kInt && done.numel() == B && done.is_contiguous(),
            "sample_tokens_full: done int32 [B]");
  SFT_CHECK(temperature > 0.0, "sample_tokens_full: temperature must be > 0");
  SFT_CHECK(repetition_penalty > 0.0, "sample_tokens_full: repetition_penalty must be > 0");
  SFT_CHECK(!tok_out.has_value() || (tok_out->is_cuda() && tok_out->scalar_type() == at::kLong &&
                                     tok_out->numel() == B && tok_out->is_contiguous()),
            "sample_tokens_full: tok int64 [B]");
  SFT_CHECK(!pos_out.has_value() ||
                (len_out.has_value() && pos_out->is_cuda() && len_out->is_cuda() && pos_out->scalar_type() == at::kLong &&
                 len_out->scalar_type() == at::kInt && pos_out->numel() == B && len_out->numel() == B &&
                 pos_out->is_contiguous() && len_out->is_contiguous()),
            "sample_tokens_full: pos int64 [B] / len int32 [B]");
  SFT_CHECK(!log.has_value() || (log->is_cuda() && log->scalar_type() == at::kLong && log->dim() == 2 &&
                                 log->size(0) == B && log->is_contiguous()), "sample_tokens_full: log int64 [B, cap]");
  SFT_CHECK(logp_log.is_cuda() && logp_log.scalar_type() == at::kFloat && logp_log.dim() == 2 && logp_log.size(0) == B &&
                logp_log.is_contiguous(), "sample_tokens_full: logp_log fp32 [B, cap]");
  const int tiles = (V + samp::TILE - 1) / samp::TILE;
  auto part = at::empty({B * tiles * 4}, logits.options().dtype(at::kFloat));
  auto part_i = at::empty({B * tiles}, logits.options().dtype(at::kInt));
  const float inv_t = (float)(1.0 / std::max(temperature, 1e-5));
  const int words = presence.size(1);
  const auto* pres = (const unsigned*)presence.data_ptr<int>();
  const auto* st = (const long long*)state.data_ptr<int64_t>();
  SFT_TRACE("samp.full");
  if (logits.scalar_type() == at::kFloat)
    samp::full_partial_kernel<float><<<dim3(tiles, B), samp::NT, 0, cur_stream()>>>(
        logits.data_ptr<float>(), V, pres, words, inv_t, (float)repetition_penalty, (unsigned)seed, st,
        part.data_ptr<float>(), part_i.data_ptr<int>(), done.data_ptr<int>());
  else
    samp::full_partial_kernel<u16><<<dim3(tiles, B), samp::NT, 0, cur_stream()>>>(
        (const u16*)logits.data_ptr(), V, pres, words, inv_t, (float)repetition_penalty, (unsigned)seed, st,
        part.data_ptr<float>(), part_i.data_ptr<int>(), done.data_ptr<int>());
  SFT_LAUNCH_CHECK();
  samp::full_final_kernel<<<B, samp::NT, 0, cur_stream()>>>(
      part.data_ptr<float>(), part_i.data_ptr<int>(), tiles, V, (long long*)state.data_ptr<int64_t>(),
      tok_out.has_value() ? (long long*)tok_out->data_ptr<int64_t>() : nullptr,
      pos_out.has_value() ? (long long*)pos_out->data_ptr<int64_t>() : nullptr,
      len_out.has_value() ? len_out->data_ptr<int>() : nullptr,
      log.has_value() ? (long long*)log->data_ptr<int64_t>() : nullptr, log.has_value() ? (int)log->size(1) : 0,
      logp_log.data_ptr<float>(), (int)logp_log.size(1), (unsigned*)presence.data_ptr<int>(), words,
      done.data_ptr<int>(), (int)eos_token_id);
  SFT_LAUNCH_CHECK();
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("sample_token", &sample_token);
  m.impl("sample_tokens", &sample_tokens);
  m.impl("sample_tokens_full", &sample_tokens_full);
}

}  // namespace sftamd
