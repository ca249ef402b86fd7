// Single-token GQA decode attention on MFMAs, head_dim 64 (Llama-3.2-1B, SmolLM2, TinyLlama, Qwen2.5-0.5B): the split
// kernels of decode_attention / decode_attention_batched at that head_dim. Outside they are the head_dim-128 kernels of
// csrc/decode_attention.hip: grid (splits, nkv[, B]) over 256-key chunks, the live length read from device memory
// (static shapes, capturable), fp32 partials (max, sum, unnormalised O) per (chunk, query head) in the same layout, an
// empty chunk written as the neutral element, the append and combine kernels shared. Inside nothing is shared: the
// kernel is a template on the head dimension; the unshared ops instantiate and bind it for 64 only, the shared-prefix
// step at the end of this file (prefix_kernel / suffix_kernel) for 64 and 128.
//
// Work split. A workgroup of four waves takes one (sequence, kv head, 256-key chunk), a wave 64 keys of it. The
// rep = nq / nkv <= 8 query heads of the GQA group are the columns of ONE 16-wide MFMA tile (columns >= rep are zeros
// that nobody stores), so K and V are read once per group and every product is a v_mfma_f32_16x16x32_bf16:
//   A[row r][k 8 g + j], B[k 8 g + j][col r], C[row 4 g + i][col r]   (g = lane >> 4, r = lane & 15, j < 8, i < 4).
//
// Scores, S^T = K Q^T: the A operand is 16 keys x 32 dims, which is lane (g, r) loading the 16 bytes at dims
// 32 ks + 8 g of key 16 t + r straight from the cache row; the B operand is the same pattern on q. Neither touches LDS.
// Per wave 4 key tiles x D / 32 k-steps. The accumulator of tile t holds keys 16 t + 4 g + {0..3} of head r: max and
// sum over the keys are 16 in-lane steps and two cross-lane ones (xor 16, 32), in the log2 domain with scale * log2(e)
// folded in. Keys >= len are -inf BEFORE the max, and no address at or past row len is ever formed: a dead lane loads
// row len - 1 (live whenever its chunk is not empty) and selects zeros, so the loads stay unconditional and all in
// flight; a wave with no live key loads nothing.
//
// P.V, O^T = V^T P^T: the B operand of key block u (32 keys) is, for lane (g, r), the four P of tile 2 u followed by the
// four of tile 2 u + 1, which are its own accumulator registers. That fixes the contraction order k = 8 g + j <-> key
// 32 u + 16 (j >> 2) + 4 g + (j & 3), and the A operand V^T is fetched in the same order by two ds_read_b64_tr_b16 from
// the wave's 64 x D tile of V in LDS (rows 32 u + 4 g + q and 32 u + 16 + 4 g + q, q = (lane & 15) >> 2, at dims
// 16 dt + 4 (lane & 3)). P is split into two bf16 halves, hi = bf16(p), lo = bf16(p - hi), two MFMAs per tile: with V
// exact in bf16 the product is as good as an fp32 P (relative error 2^-17 per term), so the output meets the per-head
// bound of the scalar head_dim-128 kernel. The row sum is taken from the fp32 p.
//
// LDS. Row `row` of a wave's V tile keeps its 16-byte chunk c at chunk c ^ 2 ((row >> s) & (D / 16 - 1)), s = 1 at
// D = 64 (two rows per 256-byte bank row), s = 0 at 128. A transposed read covers 16 consecutive rows x one aligned
// 32-byte pair: the xor sends the pairs of any 8 aligned rows to the 8 different 32-byte slots of a bank row (every bank
// twice for the 512 bytes read: the minimum). A staging write has lane l at row l / (D / 8), chunk l % (D / 8): each of
// the 16-lane groups in which a 16-byte access is serviced ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ..) writes 256
// different bytes of a bank row, since the xor only permutes chunks inside a row's own half and never moves a chunk
// across the 64-byte halves the groups alternate between on rows 2 k, 2 k + 1. A wave reads only what it wrote.
//
// Merge. Each wave leaves (m, l, O) of its 64 keys in LDS (over the V tiles, after a barrier); 256 threads merge the
// four in wave order, skipping empty waves, and write the block's partial. No atomics, every reduction in a fixed order
// that depends on nothing but the sequence's own length: the result of a sequence does not depend on B, on S_max or on
// its neighbours, and the single-sequence and batched entry points share split_body bit for bit.
//
// No sliding window (no head_dim-64 family has one; the ops raise).
#include "decode_attention_d64.h"
#include "gemm_prims.h"

namespace sftamd {
namespace decode64 {

constexpr int CHUNK = 256;  // keys per workgroup
constexpr int WKEYS = 64;   // keys per wave
constexpr int MAXREP = 8;

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <int HD>
__device__ __forceinline__ int v_off(int row, int ch) {  // byte offset of chunk ch of row `row` in a wave's V tile
  constexpr int SH = HD == 64 ? 1 : 0;
  return row * (HD * 2) + 16 * (ch ^ (((row >> SH) & (HD / 16 - 1)) << 1));
}

// 16 bytes at p + (ok ? off : safe) elements, zeros unless ok: `safe` is an offset that is always readable
__device__ __forceinline__ u32x4 load16_or_zero(const u16* __restrict__ p, long off, long safe, bool ok) {
  const u32x4 v = *(const u32x4*)(p + (ok ? off : safe));
  return ok ? v : (u32x4){0u, 0u, 0u, 0u};
}

// One (split, kv head) workgroup of one sequence; shared by the single-sequence and the batched kernel.
// q: [nq * HD] bf16; kc / vc: [S_max, nkv, HD] bf16; len in [.., S_max]; po: [rep, HD] f32; pml: [rep, 2] f32
template <int HD>
__device__ __forceinline__ void split_body(const u16* __restrict__ q, const u16* __restrict__ kc,
                                           const u16* __restrict__ vc, const int len, float* __restrict__ po,
                                           float* __restrict__ pml, const int split, const int kvh, int nq, int nkv,
                                           float sl2) {
  constexpr int KS = HD / 32;   // k-steps of a score tile
  constexpr int DT = HD / 16;   // 16-dim tiles of O^T
  constexpr int RCH = HD / 8;   // 16-byte chunks of a row
  constexpr int ROWB = HD * 2;  // bytes of a row
  constexpr int TILEB = WKEYS * ROWB;
  static_assert(HD == 64 || HD == 128, "head_dim");
  static_assert(4 * MAXREP * HD * 4 <= 4 * TILEB, "the merge buffer lies over the V tiles");
  __shared__ __attribute__((aligned(16))) char vs[4 * TILEB];  // V tiles, then the waves' O [4][MAXREP][HD] f32
  __shared__ float wml[4][MAXREP][2];
  const int rep = nq / nkv;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, r = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k0 = split * CHUNK;
  if (k0 >= len) {  // empty chunk: neutral element for the combine
    if (tid < rep) {
      pml[tid * 2] = -INFINITY;
      pml[tid * 2 + 1] = 0.f;
    }
    return;
  }
  const int kw = k0 + wave * WKEYS;  // the wave's first key
  const bool wlive = kw < len;       // wave-uniform; wave 0 is always live here
  const long rstride = (long)nkv * HD;
  const long safe = (long)(len - 1) * rstride + (long)kvh * HD;  // row len - 1 of this kv head: live
  char* vw = vs + wave * TILEB;

  u32x4 ka[4][KS], qb[KS];
  if (wlive) {
    // q: head r of the group (heads >= rep: zeros, the address clamped into the group), dims 32 ks + 8 g
    const long qoff = (long)(kvh * rep + min(r, rep - 1)) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 v = *(const u32x4*)(q + qoff + 32 * ks);
      qb[ks] = r < rep ? v : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = kw + 16 * t + r;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        ka[t][ks] = load16_or_zero(kc, (long)key * rstride + (long)kvh * HD + 32 * ks + 8 * g, safe, key < len);
    }
    // the wave's V tile -> LDS, rows past the live length as zeros (their P is zero too: 0 x 0, never 0 x NaN)
    u32x4 vr[RCH];
#pragma unroll
    for (int it = 0; it < RCH; ++it) {
      const int p = lane + 64 * it, row = p / RCH, ch = p % RCH;
      vr[it] = load16_or_zero(vc, (long)(kw + row) * rstride + (long)kvh * HD + 8 * ch, safe, kw + row < len);
    }
#pragma unroll
    for (int it = 0; it < RCH; ++it) {
      const int p = lane + 64 * it, row = p / RCH, ch = p % RCH;
      *(u32x4*)(vw + v_off<HD>(row, ch)) = vr[it];
    }
  }
  __syncthreads();

  float m = -INFINITY, l = 0.f;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (wlive) {
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        s[t] = mfma16(__builtin_bit_cast(bf16x8, ka[t][ks]), __builtin_bit_cast(bf16x8, qb[ks]), s[t]);
    }
    // s[t][i]: key kw + 16 t + 4 g + i, head r. Key kw is live, so every head's max is finite.
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = (kw + 16 * t + 4 * g + i < len) ? s[t][i] * sl2 : -INFINITY;
        m = fmaxf(m, s[t][i]);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    u32x4 phi[2], plo[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      unsigned hi[4], lo[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {  // pair h of the block's eight P: tile 2 u + (h >> 1), registers 2 (h & 1), + 1
        const int t = 2 * u + (h >> 1), i = 2 * (h & 1);
        const float p0 = exp2f(s[t][i] - m), p1 = exp2f(s[t][i + 1] - m);
        l += p0;
        l += p1;
        hi[h] = pk2bf(p0, p1);
        lo[h] = pk2bf(p0 - __uint_as_float(hi[h] << 16), p1 - __uint_as_float(hi[h] & 0xffff0000u));
      }
      phi[u] = (u32x4){hi[0], hi[1], hi[2], hi[3]};
      plo[u] = (u32x4){lo[0], lo[1], lo[2], lo[3]};
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    // V^T fragments: rows 32 u + 4 g + q (and + 16), dims 16 dt + 4 pp .. + 3
    const int qq = r >> 2, pp = r & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 32 * u + 4 * g + qq;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 vt = lds_tr<16 * ROWB>(vw, v_off<HD>(row, 2 * dt + (pp >> 1)) + 8 * (pp & 1));
        o[dt] = mfma16(vt, __builtin_bit_cast(bf16x8, phi[u]), o[dt]);
        o[dt] = mfma16(vt, __builtin_bit_cast(bf16x8, plo[u]), o[dt]);
      }
    }
  }
  __syncthreads();  // every wave is done with its V tile: the merge buffer takes its place
  float* om = (float*)vs;
  if (r < rep) {  // o[dt][i]: dim 16 dt + 4 g + i of head r
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f32x4*)(om + (wave * MAXREP + r) * HD + 16 * dt + 4 * g) = o[dt];
    if (g == 0) {
      wml[wave][r][0] = m;
      wml[wave][r][1] = l;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < rep * HD; idx += 256) {
    const int h = idx / HD, d = idx % HD;
    const float M = fmaxf(fmaxf(wml[0][h][0], wml[1][h][0]), fmaxf(wml[2][h][0], wml[3][h][0]));
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = wml[w][h][0];
      if (mw == -INFINITY) continue;
      const float f = exp2f(mw - M);
      L += f * wml[w][h][1];
      O += f * om[(w * MAXREP + h) * HD + d];
    }
    po[idx] = O;
    if (d == 0) {
      pml[h * 2] = M;
      pml[h * 2 + 1] = L;
    }
  }
}

// part_o: [nkv, splits, rep, HD] f32; part_ml: [nkv, splits, rep, 2]
template <int HD>
__global__ __launch_bounds__(256) void split_kernel(const u16* __restrict__ q, const u16* __restrict__ kc,
                                                    const u16* __restrict__ vc, const int* __restrict__ len_p,
                                                    float* __restrict__ part_o, float* __restrict__ part_ml, int nq,
                                                    int nkv, int smax, float sl2) {
  const int split = blockIdx.x, kvh = blockIdx.y, splits = gridDim.x;
  const int rep = nq / nkv;
  const long blk = (long)kvh * splits + split;
  split_body<HD>(q, kc, vc, min(*len_p, smax), part_o + blk * rep * HD, part_ml + blk * rep * 2, split, kvh, nq, nkv,
                 sl2);
}

// grid (splits, nkv, B). qkv: [B, (nq + 2 nkv) * HD]; kc / vc: [B, S_max, nkv, HD]; part_o: [B, nkv, splits, rep, HD]
template <int HD>
__global__ __launch_bounds__(256) void split_batched_kernel(const u16* __restrict__ qkv, const u16* __restrict__ kc,
                                                            const u16* __restrict__ vc, const int* __restrict__ lens,
                                                            float* __restrict__ part_o, float* __restrict__ part_ml,
                                                            int nq, int nkv, int smax, float sl2) {
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, splits = gridDim.x;
  const int rep = nq / nkv;
  // A length outside (0, S_max] is a row the append skipped: it attends over nothing (every chunk empty, zeros from
  // the combine), where the head_dim-128 kernel attends over the whole slab. Either way nothing past the slab is read.
  const int len = lens[b] <= smax ? lens[b] : 0;
  const long blk = ((long)b * nkv + kvh) * splits + split;
  const long slab = (long)b * smax * nkv * HD;
  split_body<HD>(qkv + (long)b * (nq + 2 * nkv) * HD, kc + slab, vc + slab, len, part_o + blk * rep * HD,
                 part_ml + blk * rep * 2, split, kvh, nq, nkv, sl2);
}

void launch_split(const u16* q, const u16* kc, const u16* vc, const int* len_p, float* part_o, float* part_ml, int nq,
                  int nkv, int smax, float sl2, hipStream_t st) {
  const int splits = (smax + CHUNK - 1) / CHUNK;
  split_kernel<D><<<dim3(splits, nkv), 256, 0, st>>>(q, kc, vc, len_p, part_o, part_ml, nq, nkv, smax, sl2);
  SFT_LAUNCH_CHECK();
}

void launch_split_batched(const u16* qkv, const u16* kc, const u16* vc, const int* lens, float* part_o, float* part_ml,
                          int B, int nq, int nkv, int smax, float sl2, hipStream_t st) {
  const int splits = (smax + CHUNK - 1) / CHUNK;
  split_batched_kernel<D><<<dim3(splits, nkv, B), 256, 0, st>>>(qkv, kc, vc, lens, part_o, part_ml, nq, nkv, smax, sl2);
  SFT_LAUNCH_CHECK();
}

// ---- shared prefix: the G rows of a group attend over ONE copy of their prompt's K/V ---------------------------------
//
// Rows b = grp * G + i (i < G) share prefix[grp, :plen]. Over those keys the step is one K/V stream against G * rep
// queries, so the MFMA columns are the pairs c = i * rep + h (row i of the group, head h of the kv head's GQA group),
// 16 at a time, where split_body has rep <= 8 live columns of 16. A workgroup takes one (group, kv head, 256-key chunk
// of the prefix), a wave 64 keys of it, with split_body's operand layouts. What is new is the reuse: the wave's K
// operands (4 tiles x D / 32 k-steps) are loaded once, its V tile goes through LDS once and its V^T fragments
// (2 key blocks x D / 16 tiles of ds_read_b64_tr_b16) stay in registers, so a column tile costs 16 bytes of q per
// lane and k-step, the MFMAs and the merge, and the prompt is streamed from HBM once per group instead of G times.
// With the fragments in registers LDS is free after the first barrier: the four waves' (m, l, O) of a column tile go
// where the V tiles were, 256 threads merge them in wave order exactly as split_body does and write slot `split` of
// each column's own row and head; two barriers per column tile. Columns never mix: an MFMA column depends on its own
// B operand only, the cross-lane steps (xor 16, 32) stay inside a column, the merge reads its own column. So a row's
// result does not depend on G, on its place in the tile or on what its neighbours hold (NaN included).
// Every slot of every row is written: an empty chunk (k0 >= plen, a group-wide fact) writes the neutral element.

constexpr int COLS = 16;  // columns of an MFMA tile

// own live length of row b given its total length and its group's prefix length; 0: skipped (attends over no own key)
__device__ __forceinline__ int own_len(int len, int plen, int sown) {
  const int own = len - plen;
  return own > 0 && own <= sown ? own : 0;
}

__device__ __forceinline__ int clamp_plen(int plen, int pmax) { return min(max(plen, 0), pmax); }

// grid (ceil(pmax / 256), nkv, n_groups). pk / pv: [n_groups, pmax, nkv, HD]; part_o: [B, nkv, splits_total, rep, HD]
template <int HD>
__global__ __launch_bounds__(256) void prefix_kernel(const u16* __restrict__ qkv, const u16* __restrict__ pk,
                                                     const u16* __restrict__ pv, const int* __restrict__ plens,
                                                     float* __restrict__ part_o, float* __restrict__ part_ml, int G,
                                                     int nq, int nkv, int pmax, int splits_total, float sl2) {
  constexpr int KS = HD / 32, DT = HD / 16, RCH = HD / 8, ROWB = HD * 2, TILEB = WKEYS * ROWB;
  static_assert(HD == 64 || HD == 128, "head_dim");
  static_assert(4 * COLS * HD * 4 <= 4 * TILEB, "the merge buffer lies over the V tiles");
  __shared__ __attribute__((aligned(16))) char vs[4 * TILEB];  // V tiles, then per column tile O [4][COLS][HD] f32
  __shared__ float wml[4][COLS][2];
  const int split = blockIdx.x, kvh = blockIdx.y, grp = blockIdx.z;
  const int rep = nq / nkv, ncol = G * rep;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, r = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plen = clamp_plen(plens[grp], pmax);
  const int k0 = split * CHUNK;
  // slot `split` of column c: row grp * G + c / rep, head c % rep of this kv head
  auto slot = [&](int c) { return ((((long)grp * G + c / rep) * nkv + kvh) * splits_total + split) * rep + c % rep; };
  if (k0 >= plen) {  // empty chunk: neutral element for the combine, for every row of the group
    for (int c = tid; c < ncol; c += 256) {
      part_ml[slot(c) * 2] = -INFINITY;
      part_ml[slot(c) * 2 + 1] = 0.f;
    }
    return;
  }
  const int kw = k0 + wave * WKEYS;
  const bool wlive = kw < plen;  // wave-uniform; wave 0 is always live here
  const long rstride = (long)nkv * HD;
  const u16* kc = pk + (long)grp * pmax * rstride;
  const u16* vc = pv + (long)grp * pmax * rstride;
  const long safe = (long)(plen - 1) * rstride + (long)kvh * HD;  // row plen - 1 of this kv head: live
  char* vw = vs + wave * TILEB;

  u32x4 ka[4][KS];
  bf16x8 vt[2][DT];
  if (wlive) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = kw + 16 * t + r;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        ka[t][ks] = load16_or_zero(kc, (long)key * rstride + (long)kvh * HD + 32 * ks + 8 * g, safe, key < plen);
    }
    u32x4 vr[RCH];
#pragma unroll
    for (int it = 0; it < RCH; ++it) {
      const int p = lane + 64 * it, row = p / RCH, ch = p % RCH;
      vr[it] = load16_or_zero(vc, (long)(kw + row) * rstride + (long)kvh * HD + 8 * ch, safe, kw + row < plen);
    }
#pragma unroll
    for (int it = 0; it < RCH; ++it) {
      const int p = lane + 64 * it, row = p / RCH, ch = p % RCH;
      *(u32x4*)(vw + v_off<HD>(row, ch)) = vr[it];
    }
  }
  __syncthreads();
  if (wlive) {  // V^T fragments: rows 32 u + 4 g + q (and + 16), dims 16 dt + 4 pp .. + 3, kept for every column tile
    const int qq = r >> 2, pp = r & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        vt[u][dt] = lds_tr<16 * ROWB>(vw, v_off<HD>(32 * u + 4 * g + qq, 2 * dt + (pp >> 1)) + 8 * (pp & 1));
  }
  float* om = (float*)vs;
  const long qrow = (long)(nq + 2 * nkv) * HD;
  for (int c0 = 0; c0 < ncol; c0 += COLS) {
    float m = -INFINITY, l = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (wlive) {
      // q: column c0 + r (columns >= ncol: zeros, the address clamped into the group), dims 32 ks + 8 g
      const int c = min(c0 + r, ncol - 1);
      const u16* q = qkv + ((long)grp * G + c / rep) * qrow + (long)(kvh * rep + c % rep) * HD + 8 * g;
      u32x4 qb[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const u32x4 v = *(const u32x4*)(q + 32 * ks);
        qb[ks] = c0 + r < ncol ? v : (u32x4){0u, 0u, 0u, 0u};
      }
      f32x4 s[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          s[t] = mfma16(__builtin_bit_cast(bf16x8, ka[t][ks]), __builtin_bit_cast(bf16x8, qb[ks]), s[t]);
      }
      // s[t][i]: key kw + 16 t + 4 g + i, column r. Key kw is live, so every column's max is finite.
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[t][i] = (kw + 16 * t + 4 * g + i < plen) ? s[t][i] * sl2 : -INFINITY;
          m = fmaxf(m, s[t][i]);
        }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {  // pair h of the block's eight P: tile 2 u + (h >> 1), registers 2 (h & 1), + 1
          const int t = 2 * u + (h >> 1), i = 2 * (h & 1);
          const float p0 = exp2f(s[t][i] - m), p1 = exp2f(s[t][i + 1] - m);
          l += p0;
          l += p1;
          hi[h] = pk2bf(p0, p1);
          lo[h] = pk2bf(p0 - __uint_as_float(hi[h] << 16), p1 - __uint_as_float(hi[h] & 0xffff0000u));
        }
        const bf16x8 phi = __builtin_bit_cast(bf16x8, ((u32x4){hi[0], hi[1], hi[2], hi[3]}));
        const bf16x8 plo = __builtin_bit_cast(bf16x8, ((u32x4){lo[0], lo[1], lo[2], lo[3]}));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          o[dt] = mfma16(vt[u][dt], phi, o[dt]);
          o[dt] = mfma16(vt[u][dt], plo, o[dt]);
        }
      }
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
    }
    __syncthreads();  // the V fragments are read (first tile) / the last tile's merge is done: the buffer is free
    // o[dt][i]: dim 16 dt + 4 g + i of column r
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f32x4*)(om + (wave * COLS + r) * HD + 16 * dt + 4 * g) = o[dt];
    if (g == 0) {
      wml[wave][r][0] = m;
      wml[wave][r][1] = l;
    }
    __syncthreads();
    const int live_cols = min(COLS, ncol - c0);
    for (int idx = tid; idx < live_cols * HD; idx += 256) {
      const int cl = idx / HD, d = idx % HD;
      const float M = fmaxf(fmaxf(wml[0][cl][0], wml[1][cl][0]), fmaxf(wml[2][cl][0], wml[3][cl][0]));
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float mw = wml[w][cl][0];
        if (mw == -INFINITY) continue;
        const float f = exp2f(mw - M);
        L += f * wml[w][cl][1];
        O += f * om[(w * COLS + cl) * HD + d];
      }
      const long sl = slot(c0 + cl);
      part_o[sl * HD + d] = O;
      if (d == 0) {
        part_ml[sl * 2] = M;
        part_ml[sl * 2 + 1] = L;
      }
    }
  }
}

// Row b's K and V of this step -> own cache[b, own - 1], own = lens[b] - plen of its group. One block per row.
template <int HD>
__global__ __launch_bounds__(256) void append_own_kernel(const u16* __restrict__ qkv, u16* __restrict__ kc,
                                                         u16* __restrict__ vc, const int* __restrict__ lens,
                                                         const int* __restrict__ plens, int G, int nq, int nkv,
                                                         int sown, int pmax) {
  const int b = blockIdx.x;
  const int own = own_len(lens[b], clamp_plen(plens[b / G], pmax), sown);
  if (own == 0) return;
  const int nvec = nkv * HD / 8;  // 16-byte vectors per K (and per V) row
  const u32x4* src = (const u32x4*)(qkv + (long)b * (nq + 2 * nkv) * HD + (long)nq * HD);
  const long row = ((long)b * sown + (own - 1)) * nvec;
  for (int i = threadIdx.x; i < nvec; i += 256) {
    ((u32x4*)kc)[row + i] = src[i];
    ((u32x4*)vc)[row + i] = src[nvec + i];
  }
}

// grid (ceil(sown / 256), nkv, B): split_body over row b's own slab, into the slots after the prefix's
template <int HD>
__global__ __launch_bounds__(256) void suffix_kernel(const u16* __restrict__ qkv, const u16* __restrict__ kc,
                                                     const u16* __restrict__ vc, const int* __restrict__ lens,
                                                     const int* __restrict__ plens, float* __restrict__ part_o,
                                                     float* __restrict__ part_ml, int G, int nq, int nkv, int sown,
                                                     int pmax, int psplits, int splits_total, float sl2) {
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int rep = nq / nkv;
  const int own = own_len(lens[b], clamp_plen(plens[b / G], pmax), sown);
  const long blk = ((long)b * nkv + kvh) * splits_total + psplits + split;
  const long slab = (long)b * sown * nkv * HD;
  split_body<HD>(qkv + (long)b * (nq + 2 * nkv) * HD, kc + slab, vc + slab, own, part_o + blk * rep * HD,
                 part_ml + blk * rep * 2, split, kvh, nq, nkv, sl2);
}

template <int HD>
static void prefix_step(const u16* qkv, u16* kc, u16* vc, const int* lens, const u16* pk, const u16* pv,
                        const int* plens, float* part_o, float* part_ml, int B, int G, int nq, int nkv, int sown,
                        int pmax, float sl2, hipStream_t st) {
  const int psplits = (pmax + CHUNK - 1) / CHUNK, osplits = (sown + CHUNK - 1) / CHUNK;
  append_own_kernel<HD><<<B, 256, 0, st>>>(qkv, kc, vc, lens, plens, G, nq, nkv, sown, pmax);
  SFT_LAUNCH_CHECK();
  prefix_kernel<HD><<<dim3(psplits, nkv, B / G), 256, 0, st>>>(qkv, pk, pv, plens, part_o, part_ml, G, nq, nkv, pmax,
                                                               psplits + osplits, sl2);
  SFT_LAUNCH_CHECK();
  suffix_kernel<HD><<<dim3(osplits, nkv, B), 256, 0, st>>>(qkv, kc, vc, lens, plens, part_o, part_ml, G, nq, nkv, sown,
                                                           pmax, psplits, psplits + osplits, sl2);
  SFT_LAUNCH_CHECK();
}

void launch_prefix_step(int hd, const u16* qkv, u16* kc, u16* vc, const int* lens, const u16* pk, const u16* pv,
                        const int* plens, float* part_o, float* part_ml, int B, int G, int nq, int nkv, int sown,
                        int pmax, float sl2, hipStream_t st) {
  if (hd == 64)
    prefix_step<64>(qkv, kc, vc, lens, pk, pv, plens, part_o, part_ml, B, G, nq, nkv, sown, pmax, sl2, st);
  else
    prefix_step<128>(qkv, kc, vc, lens, pk, pv, plens, part_o, part_ml, B, G, nq, nkv, sown, pmax, sl2, st);
}

}  // namespace decode64
}  // namespace sftamd
