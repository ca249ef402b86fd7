// Offline distillation over a 128k vocabulary for gfx950: the teacher's top-K log-probabilities per token row
// (teacher_topk, computed once per dataset and cached) and the student's forward KL against such a truncated teacher
// (kd_topk_fwd; twins: ops/reference.py teacher_topk / distill_topk / distill_topk_grad).
//
// Both kernels are one 256-thread block per token row with 16-byte loads, the online accumulator, block combine and
// rows-in-flight cap of vocab_rows.h (shared with ce_fwd and kd_fwd); the sweep here visits ONE row.
//
// teacher_topk. Exact selection, not a sort of the row: a bf16 logit has 65,536 possible values, so the K-th largest
// is found by a two-level 8-bit histogram of an order-preserving 16-bit key in LDS, and the K entries are then
// collected and ranked in LDS. Integer LDS counters are order-independent, and every slot of the result is decided
// by (key, column) alone, so the output is the same in every run. Passes over the row (the first from HBM, the others
// from the cache: the launch caps the rows in flight):
//   A  online (max, sum) of x / tau for the row's lse, and every thread's own maximum. The K-th largest of the 256
//      thread maxima is a floor F with at least K elements >= F, so nothing below F can be among the top K: the passes
//      below look only at elements >= F (about 1 % of a 128k row), which keeps the LDS atomics off the critical path
//   B  histogram of the key's high byte            -> the high byte of the K-th key, the count above it
//   C  histogram of the low byte within that bin   -> the K-th key, n_gt elements above it, n_eq equal to it
//   D  elements above the K-th key (and the equal ones when all n_eq are taken) go to LDS slots handed out by a counter
//   E  only when fewer than n_eq equal elements are taken: the lowest columns first. Rounds of 256 vectors in column
//      order, a block prefix count per round, ends as soon as enough are found
// then thread i ranks entry i among the K (key descending, column ascending) and writes (column, x / tau - lse) there.
// Order: value descending, equal values by column ascending (-0 and +0 are equal) = torch.sort(x.float(),
// descending=True, stable=True)[:K]. The logits are finite and only read.
//
// kd_topk_fwd. With a = s / tau, lp = a - lse(a), the cached (id_k, tlp_k), p_k = e^tlp_k and m = sum_k p_k, per valid row:
//   L = sum_k p_k (tlp_k - lp[id_k])        dL/da_j = m e^lp_j - sum_k [id_k = j] p_k
// the forward KL truncated to the teacher's top-K support, not renormalised (K = V: kd_fwd's KD_FKL). Thread k < K
// gathers a[id_k] before anything is written; pass 1 is the student's online (max, sum, argmax); L and m are summed in
// one fixed order (wave butterfly, then waves 0..3). The gradient pass overwrites the student's row with bf16
// (m e^lp_j) * inv_count / tau; after a block barrier thread k stores element id_k again as bf16
// (m e^lp[id_k] - p_k) * inv_count / tau, computed from its gathered logit: one rounding, nothing read back.
// The ids of a row are distinct and in [0, V): a caller error otherwise (SFT_DASSERT in the debug build; the release
// kernel skips an out-of-range id, duplicates leave the last writer's value).
#include "vocab_rows.h"

#include <cmath>
#include <cstdlib>

namespace sftamd {

constexpr int kTopkMax = 256;              // K <= the block's threads: thread k owns entry k
constexpr int kTopkStaticLds = 6 * 1024;   // teacher_topk_kernel's static LDS, rounded up (taken off the row pad)

// The row loop of a pass over one row: vocab_rows.h's sweep_row_pair with one stream. body(raw, v).
template <int U, class Body>
__device__ __forceinline__ void sweep_row(const u16* r, int nvec, int tid, Body&& body) {
  int v = tid;
  for (; v + 256 * (U - 1) < nvec; v += 256 * U) {
    uint4 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = *(const uint4*)(r + (long)(v + 256 * u) * 8);
#pragma unroll
    for (int u = 0; u < U; ++u) body(a[u], v + 256 * u);
  }
  for (; v < nvec; v += 256) body(*(const uint4*)(r + (long)v * 8), v);
}

// Eight scaled elements into the online accumulator (kd_fwd's kd_accum without a numerator): max, sum, first argmax.
__device__ __forceinline__ void topk_accum(RowAcc& acc, const float* x, int base) {
  float mx = x[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) mx = fmaxf(mx, x[i]);
  const float M = fmaxf(acc.m, mx);
  const float sc = __expf(acc.m - M);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s += __expf(x[i] - M);
    if (x[i] > acc.bv) {
      acc.bv = x[i];
      acc.bi = base + i;
    }
  }
  acc.s = acc.s * sc + s;
  acc.m = M;
}

// The 16 raw bits of a bf16 as a 16-bit key that orders like the value (-0 = +0).
__device__ __forceinline__ unsigned topk_key(unsigned u) {
  u = (u == 0x8000u) ? 0u : u;
  return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

__device__ __forceinline__ void raw8(const uint4& v, unsigned* u) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[2 * i] = w[i] & 0xffffu;
    u[2 * i + 1] = w[i] >> 16;
  }
}

// hist[0..255] -> the bin of the kk-th largest entry and the count above that bin (one thread finds both).
__device__ __forceinline__ void topk_find_bin(const unsigned* hist, int kk, int tid, int* bin, int* above) {
  int s = 0;
  for (int j = tid + 1; j < 256; ++j) s += (int)hist[j];
  if (s < kk && s + (int)hist[tid] >= kk) {
    *bin = tid;
    *above = s;
  }
}

template <int U>
__global__ __launch_bounds__(256) void teacher_topk_kernel(const u16* __restrict__ logits, int* __restrict__ ids,
                                                           float* __restrict__ logps, int V, int K, float inv_tau) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const u16* lr = logits + (long)row * V;
  const int nvec = V / 8;

  __shared__ float sh_tmax[256];
  __shared__ unsigned sh_hist[256];
  __shared__ unsigned sh_ckey[kTopkMax];
  __shared__ int sh_cidx[kTopkMax];
  __shared__ RowAcc red[4];
  __shared__ float sh_lse, sh_floor;
  __shared__ int sh_bin[2], sh_above[2], sh_cnt;  // [level]; 0 unless a thread finds the bin (a row with NaNs)
  __shared__ int sh_wtot[2][4];
  static_assert(sizeof(sh_tmax) + sizeof(sh_hist) + sizeof(sh_ckey) + sizeof(sh_cidx) + sizeof(red) + sizeof(sh_lse) +
                        sizeof(sh_floor) + sizeof(sh_bin) + sizeof(sh_above) + sizeof(sh_cnt) + sizeof(sh_wtot) + 256 <=
                    kTopkStaticLds,
                "kTopkStaticLds must cover this kernel's static LDS (with room for alignment)");

  auto scaled = [&](const uint4& raw, float* x) {
    unpack8(raw, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] *= inv_tau;
  };

  // ---- pass A: the row's lse and the threads' maxima
  RowAcc acc = row_acc_empty();
  sweep_row<U>(lr, nvec, tid, [&](const uint4& raw, int v) {
    float a[8];
    scaled(raw, a);
    topk_accum(acc, a, v * 8);
  });
  const float tmax = acc.m;  // -inf: a thread without a vector (V < 2048)
  sh_tmax[tid] = tmax;
  sh_hist[tid] = 0u;
  if (tid < 2) sh_bin[tid] = sh_above[tid] = 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) row_merge(acc, row_shfl_xor(acc, o));
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    RowAcc a = red[0];
    for (int w = 1; w < 4; ++w) row_merge(a, red[w]);
    sh_lse = a.m + __logf(a.s);
    sh_cnt = 0;
  }
  {  // the K-th largest thread maximum: ranks are a permutation of 0..255, so one thread writes
    int rank = 0;
    for (int j = 0; j < 256; ++j) {
      const float vj = sh_tmax[j];
      rank += (vj > tmax || (vj == tmax && j < tid)) ? 1 : 0;
    }
    if (rank == K - 1) sh_floor = tmax;
  }
  __syncthreads();
  const float F = sh_floor;
  const float lse = sh_lse;

  // ---- pass B: the high byte of the K-th key
  sweep_row<U>(lr, nvec, tid, [&](const uint4& raw, int) {
    float a[8];
    unsigned u[8];
    scaled(raw, a);
    raw8(raw, u);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (a[i] >= F) atomicAdd(&sh_hist[topk_key(u[i]) >> 8], 1u);
  });
  __syncthreads();
  topk_find_bin(sh_hist, K, tid, &sh_bin[0], &sh_above[0]);
  __syncthreads();
  const unsigned b1 = (unsigned)sh_bin[0];
  const int above1 = sh_above[0];
  sh_hist[tid] = 0u;
  __syncthreads();

  // ---- pass C: its low byte
  sweep_row<U>(lr, nvec, tid, [&](const uint4& raw, int) {
    float a[8];
    unsigned u[8];
    scaled(raw, a);
    raw8(raw, u);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (a[i] >= F) {
        const unsigned key = topk_key(u[i]);
        if ((key >> 8) == b1) atomicAdd(&sh_hist[key & 255u], 1u);
      }
  });
  __syncthreads();
  topk_find_bin(sh_hist, K - above1, tid, &sh_bin[1], &sh_above[1]);
  __syncthreads();
  const unsigned kth = (b1 << 8) | (unsigned)sh_bin[1];
  const int n_gt = above1 + sh_above[1];
  const int n_eq = (int)sh_hist[sh_bin[1]];
  const int need = K - n_gt;  // 1 <= need <= n_eq
  const bool all_eq = need >= n_eq;

  // ---- pass D: everything above the K-th key, and the equal elements when all of them are taken
  sweep_row<U>(lr, nvec, tid, [&](const uint4& raw, int v) {
    float a[8];
    unsigned u[8];
    scaled(raw, a);
    raw8(raw, u);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (a[i] >= F) {
        const unsigned key = topk_key(u[i]);
        if (key > kth || (all_eq && key == kth)) {
          const int slot = atomicAdd(&sh_cnt, 1);
          if (slot < kTopkMax) {
            sh_ckey[slot] = key;
            sh_cidx[slot] = v * 8 + i;
          }
        }
      }
  });

  // ---- pass E: the `need` lowest columns among the equal elements, into slots n_gt ..
  if (!all_eq) {
    int running = 0;
    for (int r = 0; r * 256 < nvec && running < need; ++r) {
      const int v = r * 256 + tid;
      unsigned mask = 0u;
      if (v < nvec) {
        unsigned u[8];
        raw8(*(const uint4*)(lr + (long)v * 8), u);
#pragma unroll
        for (int i = 0; i < 8; ++i) mask |= (topk_key(u[i]) == kth ? 1u : 0u) << i;
      }
      const int c = __popc(mask);
      int inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
      }
      if (lane == 63) sh_wtot[r & 1][wave] = inc;
      __syncthreads();
      int ord = running + inc - c;
      int tot = 0;
      for (int w = 0; w < 4; ++w) {
        const int t = sh_wtot[r & 1][w];
        if (w < wave) ord += t;
        tot += t;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((mask >> i) & 1u) {
          if (ord < need) {
            sh_ckey[n_gt + ord] = kth;
            sh_cidx[n_gt + ord] = v * 8 + i;
          }
          ++ord;
        }
      running += tot;
    }
  }
  __syncthreads();

  // ---- the K entries in order
  if (tid < K) {
    const unsigned key = sh_ckey[tid];
    SFT_DASSERT(sh_cidx[tid] >= 0 && sh_cidx[tid] < V);
    const int idx = min(max(sh_cidx[tid], 0), V - 1);  // (a slot nobody filled: a row with NaNs)
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const unsigned kj = sh_ckey[j];
      rank += (kj > key || (kj == key && sh_cidx[j] < idx)) ? 1 : 0;
    }
    ids[(long)row * K + rank] = idx;
    logps[(long)row * K + rank] = bf2f(lr[idx]) * inv_tau - lse;
  }
}

template <int U>
__global__ __launch_bounds__(256) void kd_topk_fwd_kernel(u16* __restrict__ student, const int* __restrict__ ids,
                                                          const float* __restrict__ logps,
                                                          const int64_t* __restrict__ labels,
                                                          const float* __restrict__ inv_count,
                                                          float* __restrict__ stats, int M, int V, int K,
                                                          int write_grad, float inv_tau) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  u16* sr = student + (long)row * V;
  const long label = labels[row];
  SFT_DASSERT(label == -100 || (label >= 0 && label < V));
  const bool valid = label >= 0 && label < V;
  const int nvec = V / 8;

  // ---- thread k's cached entry and the student's logit there, before anything is written
  int id = -1;
  float tlp = 0.f, pk = 0.f, ak = 0.f;
  bool has = false;
  if (tid < K) {
    id = ids[(long)row * K + tid];
    tlp = logps[(long)row * K + tid];
    SFT_DASSERT(!valid || (id >= 0 && id < V));
    has = id >= 0 && id < V;
    if (has) {
      ak = bf2f(sr[id]) * inv_tau;
      pk = __expf(tlp);
    }
#ifdef SFTAMD_DEBUG
    if (valid)
      for (int j = 0; j < tid; ++j) SFT_DASSERT(ids[(long)row * K + j] != id);
#endif
  }

  // ---- pass 1: the student's online (max, sum, argmax)
  RowAcc acc = row_acc_empty();
  sweep_row<U>(sr, nvec, tid, [&](const uint4& raw, int v) {
    float a[8];
    unpack8(raw, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] *= inv_tau;
    topk_accum(acc, a, v * 8);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) row_merge(acc, row_shfl_xor(acc, o));
  __shared__ RowAcc red[4];
  __shared__ float red_l[4], red_m[4];
  __shared__ float sh_lse, sh_mass;
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  RowAcc top = red[0];  // (thread 0's copy is the one used)
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) row_merge(top, red[w]);
    sh_lse = top.m + __logf(top.s);
  }
  __syncthreads();
  const float lse = sh_lse;

  // ---- the K terms of the loss and of the teacher's mass, in one fixed order
  const float lpk = ak - lse;
  float term = has ? pk * (tlp - lpk) : 0.f;
  float mass = has ? pk : 0.f;
  term = wave_sum(term);
  mass = wave_sum(mass);
  if (lane == 0) {
    red_l[wave] = term;
    red_m[wave] = mass;
  }
  __syncthreads();
  if (tid == 0) {
    const float L = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    const float m = (red_m[0] + red_m[1]) + (red_m[2] + red_m[3]);
    stats[row] = valid ? L : 0.f;
    stats[M + row] = lse;
    stats[2 * M + row] = m;
    stats[3 * M + row] = (valid && top.bi == label) ? 1.f : 0.f;
    stats[4 * M + row] = (valid && top.bi == id) ? 1.f : 0.f;
    sh_mass = m;
  }
  __syncthreads();
  if (!write_grad) return;

  // ---- gradient pass (a label-masked row: +0 in every element)
  if (!valid) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int v = tid; v < nvec; v += 256) *(uint4*)(sr + (long)v * 8) = zero;
    return;
  }
  const float m = sh_mass;
  const float scale = inv_count[0] * inv_tau;
  sweep_row<U>(sr, nvec, tid, [&](const uint4& raw, int v) {
    float a[8];
    unpack8(raw, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (m * __expf(a[i] * inv_tau - lse)) * scale;
    *(uint4*)(sr + (long)v * 8) = pack8(a);
  });
  __syncthreads();  // the row is written: the K corrected elements go over it
  if (has) sr[id] = f2bf((m * __expf(lpk) - pk) * scale);
}

// Rows in flight while the gradient is written, in MB (see kd_topk_fwd): SFTAMD_KD_TOPK_INFLIGHT_MB overrides the
// default (tools/bench_kd.py measures with it).
static long kd_topk_inflight_mb() {
  static long mb = [] {
    const char* e = std::getenv("SFTAMD_KD_TOPK_INFLIGHT_MB");
    const long v = e && e[0] ? std::atol(e) : 0;
    return v > 0 ? v : 200L;
  }();
  return mb;
}

// Rows in flight of teacher_topk, in MB: SFTAMD_TEACHER_TOPK_INFLIGHT_MB overrides the default (tools/bench_kd.py).
static long teacher_topk_inflight_mb() {
  static long mb = [] {
    const char* e = std::getenv("SFTAMD_TEACHER_TOPK_INFLIGHT_MB");
    const long v = e && e[0] ? std::atol(e) : 0;
    return v > 0 ? v : 200L;
  }();
  return mb;
}

std::tuple<at::Tensor, at::Tensor> teacher_topk(const at::Tensor& logits, int64_t k, double temperature) {
  SFT_CHECK_CUDA(logits);
  SFT_CHECK_BF16(logits);
  SFT_CHECK_CONTIG(logits);
  SFT_CHECK(logits.dim() >= 1, "teacher_topk: logits must be [M, vocab]");
  SFT_CHECK(temperature > 0.0 && std::isfinite(temperature), "teacher_topk: temperature must be > 0");
  const long Vl = logits.size(-1);
  SFT_CHECK(Vl > 0 && Vl % 8 == 0 && Vl <= INT_MAX, "vocab must be a multiple of 8");
  const int V = (int)Vl;
  SFT_CHECK(k >= 1 && k <= kTopkMax && k <= V, "teacher_topk: k must be in 1 .. min(", kTopkMax, ", vocab), got ", k);
  const long Ml = logits.numel() / V;
  SFT_CHECK(Ml <= INT_MAX, "teacher_topk: too many rows");
  const int M = (int)Ml;
  auto ids = at::empty({M, k}, logits.options().dtype(at::kInt));
  auto lps = at::empty({M, k}, logits.options().dtype(at::kFloat));
  if (M == 0) return {ids, lps};
  // The rows-in-flight cap (vocab_rows.h) at ce_fwd's budget: passes B to E re-read the row. This kernel's static LDS
  // comes off the pad, which is sized for kernels with next to none.
  const int pad = std::max(0, rows_in_flight_pad((long)V * 2, teacher_topk_inflight_mb()) - kTopkStaticLds);
  if (pad > 64 * 1024) {  // (allow_row_pad asks for the whole CU less 1 KB, more than fits next to this kernel's static LDS)
    static bool attr = hipFuncSetAttribute((const void*)teacher_topk_kernel<4>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           kMaxRowPad - kTopkStaticLds) == hipSuccess;
    SFT_CHECK(attr, "teacher_topk: could not raise the dynamic LDS limit");
  }
  SFT_TRACE("teacher_topk");
  teacher_topk_kernel<4><<<M, 256, pad, cur_stream()>>>((const u16*)logits.data_ptr(), ids.data_ptr<int>(),
                                                        lps.data_ptr<float>(), V, (int)k,
                                                        (float)(1.0 / temperature));
  SFT_LAUNCH_CHECK();
  return {ids, lps};
}

at::Tensor kd_topk_fwd(at::Tensor student_logits, const at::Tensor& ids, const at::Tensor& logps,
                       const at::Tensor& labels, const at::Tensor& inv_count, bool write_grad, double temperature) {
  SFT_CHECK_CUDA(student_logits);
  SFT_CHECK_CUDA(ids);
  SFT_CHECK_CUDA(logps);
  SFT_CHECK_BF16(student_logits);
  SFT_CHECK_CONTIG(student_logits);
  SFT_CHECK_CONTIG(ids);
  SFT_CHECK_CONTIG(logps);
  SFT_CHECK(ids.scalar_type() == at::kInt, "kd_topk_fwd: ids must be int32");
  SFT_CHECK(logps.scalar_type() == at::kFloat, "kd_topk_fwd: logps must be fp32");
  SFT_CHECK(ids.device() == student_logits.device() && logps.device() == student_logits.device(),
            "kd_topk_fwd: tensors on two devices");
  SFT_CHECK(labels.scalar_type() == at::kLong && labels.is_cuda(), "labels must be an int64 GPU tensor");
  SFT_CHECK(inv_count.scalar_type() == at::kFloat && inv_count.is_cuda() && inv_count.numel() >= 1,
            "inv_count must be a fp32 GPU tensor");
  SFT_CHECK(temperature > 0.0 && std::isfinite(temperature), "kd_topk_fwd: temperature must be > 0");
  SFT_CHECK(student_logits.dim() >= 1, "kd_topk_fwd: student_logits must be [M, vocab]");
  const long Vl = student_logits.size(-1);
  SFT_CHECK(Vl > 0 && Vl % 8 == 0 && Vl <= INT_MAX, "vocab must be a multiple of 8");
  const int V = (int)Vl;
  const long Ml = student_logits.numel() / V;
  SFT_CHECK(Ml <= INT_MAX / 5, "kd_topk_fwd: too many rows");
  const int M = (int)Ml;
  SFT_CHECK(ids.dim() == 2 && ids.size(0) == M && ids.sizes() == logps.sizes(),
            "kd_topk_fwd: ids and logps must both be [rows, k]");
  const long K = ids.size(1);
  SFT_CHECK(K >= 1 && K <= kTopkMax && K <= V, "kd_topk_fwd: k must be in 1 .. min(", kTopkMax, ", vocab), got ", K);
  SFT_CHECK(labels.numel() == M, "labels size");
  auto lab = labels.contiguous();
  auto stats = at::empty({5, M}, student_logits.options().dtype(at::kFloat));
  if (M == 0) return stats;
  // The rows-in-flight cap (vocab_rows.h): the gradient pass re-reads ONE row of 2 V bytes, ce_fwd's situation, so
  // ce_fwd's budget (3 blocks per CU at V = 128,256). The stats-only call (eval) keeps full occupancy.
  const int pad = write_grad ? rows_in_flight_pad((long)V * 2, kd_topk_inflight_mb()) : 0;
  allow_row_pad<kd_topk_fwd_kernel<4>>(pad, "kd_topk_fwd");
  SFT_TRACE("kd_topk_fwd");
  kd_topk_fwd_kernel<4><<<M, 256, pad, cur_stream()>>>((u16*)student_logits.data_ptr(), ids.data_ptr<int>(),
                                                       logps.data_ptr<float>(), lab.data_ptr<int64_t>(),
                                                       inv_count.data_ptr<float>(), stats.data_ptr<float>(), M, V,
                                                       (int)K, write_grad ? 1 : 0, (float)(1.0 / temperature));
  SFT_LAUNCH_CHECK();
  return stats;
}

TORCH_LIBRARY_IMPL(sftamd, CUDA, m) {
  m.impl("teacher_topk", &teacher_topk);
  m.impl("kd_topk_fwd", &kd_topk_fwd);
}

}  // namespace sftamd
