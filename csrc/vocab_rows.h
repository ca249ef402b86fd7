// What the one-block-per-row kernels over a 128k vocabulary share (cross_entropy.hip, distill.hip): the online
// softmax accumulator with its merge and shuffle, the sweep over a pair of rows, and the host side of the
// rows-in-flight cap. A new objective on the LM head brings its own per-vector accumulation and gradient expression.
#pragma once

#include "common.h"

#include <algorithm>
#include <climits>

namespace sftamd {

struct RowAcc {
  float m, s, t;  // running max, sum e^(x-m), one auxiliary sum of e^(x-m) * (something) the objective defines
  float bv;       // best value
  int bi;         // best index (first occurrence)
};

__device__ __forceinline__ RowAcc row_acc_empty() { return {-INFINITY, 0.f, 0.f, -INFINITY, INT_MAX}; }

__device__ __forceinline__ void row_merge(RowAcc& a, const RowAcc& b) {
  const float M = fmaxf(a.m, b.m);
  const float ea = (a.m == -INFINITY) ? 0.f : __expf(a.m - M);
  const float eb = (b.m == -INFINITY) ? 0.f : __expf(b.m - M);
  a.s = a.s * ea + b.s * eb;
  a.t = a.t * ea + b.t * eb;
  a.m = M;
  if (b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi)) {
    a.bv = b.bv;
    a.bi = b.bi;
  }
}

__device__ __forceinline__ RowAcc row_shfl_xor(const RowAcc& a, int o) {
  RowAcc b;
  b.m = __shfl_xor(a.m, o, 64);
  b.s = __shfl_xor(a.s, o, 64);
  b.t = __shfl_xor(a.t, o, 64);
  b.bv = __shfl_xor(a.bv, o, 64);
  b.bi = __shfl_xor(a.bi, o, 64);
  return b;
}

// The block combine of a 256-thread block is written out in each kernel, in one fixed order the results depend on: the
// xor butterfly per wave, row_merge(acc, row_shfl_xor(acc, o)) for o = 32 .. 1; each wave's lane 0 writes red[wave]; a
// __syncthreads; thread 0 merges red[0 .. 3] in order. It stays in the kernels, and so does ce_fwd_kernel's row loop,
// because row_merge's a * ea + b * eb leaves the compiler the choice of the product it fuses into the fma, and that
// choice follows how neighbouring merges pair up into packed math: behind a helper call the merges of ce_fwd and of
// kd_fwd's forward KL paired differently and their stats moved in the last bit (profiles/lm_head_refactor.md).

// The row loop of a pass over a pair of rows: thread tid of 256 visits the 16-byte vectors tid, tid + 256, ... of both
// rows (nvec vectors each), U independent loads per row in flight before any of them is consumed — one load per
// iteration leaves the row stream latency-bound (~3.5 TB/s) — then the tail one vector at a time.
// body(raw_a, raw_b, v), v the vector's index in the row.
template <int U, class Body>
__device__ __forceinline__ void sweep_row_pair(const u16* ra, const u16* rb, int nvec, int tid, Body&& body) {
  int v = tid;
  for (; v + 256 * (U - 1) < nvec; v += 256 * U) {
    uint4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = *(const uint4*)(ra + (long)(v + 256 * u) * 8);
      b[u] = *(const uint4*)(rb + (long)(v + 256 * u) * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) body(a[u], b[u], v + 256 * u);
  }
  for (; v < nvec; v += 256) body(*(const uint4*)(ra + (long)v * 8), *(const uint4*)(rb + (long)v * 8), v);
}

// The rows-in-flight cap. A pass that re-reads its row finds it in the 256 MB Infinity Cache only while the rows in
// flight fit it, so a launch that writes the gradient caps the blocks per CU by reserving dynamic LDS (nothing is
// stored in it) until blocks x CUs x row_bytes stays near budget_mb; 0: eight blocks fit, no cap. The budget is the
// kernel's own, measured (ce_fwd, kd_fwd).
constexpr int kMaxRowPad = 160 * 1024 - 1024;  // one block per CU; with the kernels' static scratch (under 1 KB): 160 KB

inline int rows_in_flight_pad(long row_bytes, long budget_mb) {
  const long bpc = std::max(1L, std::min(8L, (budget_mb << 20) / ((long)num_cus() * row_bytes)));
  return bpc < 8 ? (int)((160L * 1024) / bpc - 1024) : 0;
}

// Before the launch of KERNEL with ``pad`` bytes of dynamic LDS: the pad passes 64 KB once two blocks per CU remain
// (ce_fwd: V above ~136K), and a launch above 64 KB needs the limit raised first. The limit is a per-kernel attribute,
// so each instantiation that meets such a pad raises its own, once, to the largest pad.
template <auto KERNEL>
inline void allow_row_pad(int pad, const char* op) {
  SFT_CHECK(pad <= kMaxRowPad, op, ": LDS pad over the CU's 160 KB");
  if (pad > 64 * 1024) {
    static bool attr = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           kMaxRowPad) == hipSuccess;
    SFT_CHECK(attr, op, ": could not raise the dynamic LDS limit");
  }
}

}  // namespace sftamd
