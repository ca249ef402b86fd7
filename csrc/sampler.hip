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

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("sample_token", &sample_token);
  m.impl("sample_tokens", &sample_tokens);
}

}  // namespace sftamd
