// Varlen GQA flash-attention forward / backward for head_dim 64 on gfx950 (Llama-3.2-1B, SmolLM2, TinyLlama,
// Qwen2.5-0.5B). Same packed layout as csrc/attention.hip: qkv[M, (nq + 2 nkv) * 64] bf16 token-major, sequences
// [cu[b], cu[b+1]); out[M, nq * 64] bf16, lse[nq, M] fp32 (natural log), dqkv packed. bf16 I/O, fp32 accumulation,
// v_mfma_f32_32x32x16_bf16 everywhere. No sliding window here (none of the head_dim-64 families has one).
//
// LDS images. A head row is 128 B, half a bank row, so a 64-row tile (keys, or queries) is stored as 32 image rows of
// 256 B: image row r holds tile row r in its 16-byte chunks 0..7 and tile row r + 32 in chunks 8..15. With that pairing
// the 32-row block b of the tile (b = 0, 1) is the column half b of a [32][128] image, every fragment read of the
// 32x32x16 kernels is a read pattern of the head_dim-128 images (k-step 4 b + s of a row read, column block 2 b + db
// of a transposed read), and swz256_s stays conflict-free for the 16-byte row reads and for ds_read_b64_tr_b16
// (tools/lds_swizzle_check.py, attn_d64_ok). Tiles arrive by LDS-DMA through buffer descriptors (8 x 1 KB pieces per
// image, the swizzle and the row pairing applied on the source address): rows past the sequence end are outside the
// descriptor's range and read as ZERO, nothing outside the sequence's rows is ever addressed.
//
// Kernels:
// * fwd_kernel: S^T = K Q^T with the query on the lane (row max / sum lane-local + one permlane32 swap), P^T fed to
//   O^T += V^T P^T straight from the accumulator, the scale folded into the exponent, masks only on diagonal / last
//   tiles, deferred rescale THR. A workgroup = 4 waves = HW query heads of one kv head x (4 / HW) 32-query blocks
//   (HW = gcd(rep, 4)) sharing each 64-key K / V tile, two stages. Against head_dim 128 a tile is half the MFMA work
//   for the same exp / max / sum VALU work, and O^T is 32 instead of 64 accumulators: the kernel keeps 64-key tiles
//   (32 KB of LDS per workgroup, not 64) and fits 126 VGPRs, so up to four workgroups share a CU (head_dim 128: two)
//   and another wave's MFMAs run under this wave's softmax.
// * delta_kernel: rowsum(dO . O), 8 lanes per (token, head) row.
// * bwd_dkdv_kernel: 64 keys of one kv head per workgroup = 2 key halves x G head groups (G = 2 when rep is even); S
//   and dP with the KEY on the lane (K and V fragments are loop-invariant B operands in registers), P / dS as the
//   register B operands of dV^T += dO^T P and dK^T += Q^T dS; 64-query Q / dO tiles by LDS-DMA in two stages per group;
//   every query head of the kv head accumulates into the one dK / dV, the two groups are summed through LDS at the end
//   in a fixed order (no atomics).
// * bwd_dq_kernel: the forward's split (query on the lane, K / V tiles shared by the workgroup); S^T and dP^T are
//   RECOMPUTED from Q, dO, lse, delta, and dQ^T += K^T dS^T with dS^T fed from the accumulator. No atomics.
//
// Why both backward kernels recompute (head_dim 128 stores dS^T up to SFTAMD_ATTN_DS_MB): the stored dS^T costs the
// same bytes per score at any head_dim (write + read of nseq x nq x L^2 bf16), while recomputing S and dP costs two
// products of depth 64 — half of what they cost at 128, and 16 of the dQ kernel's 24 MFMAs per tile. At head_dim 64
// the traffic is the larger term, and the single design has no scratch that grows with max_seqlen^2 and no second path
// to test.
//
// v_mfma_f32_32x32x16_bf16 lane maps (hi = lane >> 5, c = lane & 31, j = 0..7, i = 0..15):
//   A[row c][k 8hi+j], B[k 8hi+j][col c], C[row crow(i, hi)][col c], crow(i, hi) = (i & 3) + 8 (i >> 2) + 4 hi.
// Accumulator registers 8 sub .. 8 sub + 7 hold rows 16 sub + 4 hi + {0..3} and 16 sub + 8 + 4 hi + {0..3}: the k order
// in which the transposed reads fetch the A operand of the next product (two ds_read_b64_tr_b16).
//
// The small helpers below (descriptor, packing, permlane reductions) repeat those of attention.hip, which keeps its
// own: the two files share only gemm_prims.h.
#include "attention_d64.h"
#include "gemm_prims.h"

namespace sftamd {
namespace attn64 {

constexpr int HROWB = D * 2;      // bytes of one head row in global memory
constexpr int ROWB = 2 * HROWB;   // bytes of one image row (two head rows)
constexpr int TB = 32 * ROWB;     // a 64-row tile image
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float THR = 8.f;  // deferred rescale: O / l are rescaled only when the row max grows by more than 2^THR

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ int swz(int row, int ch) { return swz256_s(row, ch); }
__device__ __forceinline__ int img_off(int row, int ch) { return row * ROWB + 16 * swz(row, ch); }

__device__ __forceinline__ f32x16 mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void vm_drain() { __builtin_amdgcn_s_waitcnt(waitcnt_imm(0, 15)); }

// [p, p + bytes) as a raw buffer: offsets past the range read as zero
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, long bytes) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const unsigned n = __builtin_amdgcn_readfirstlane((unsigned)(bytes < 0 ? 0 : bytes));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, n, 0x00020000);
}
__device__ __forceinline__ bf16x8 bload16(rsrc_t r, unsigned voff) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
__device__ __forceinline__ bf16x8 lds_tr2(const char* base, int lo, int hi) {
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + lo));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + hi));
  s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 pack_acc(const f32x16& t, int base) {  // t[base .. base + 7] as 8 bf16
  return __builtin_bit_cast(bf16x8, u32x4{pk2bf(t[base], t[base + 1]), pk2bf(t[base + 2], t[base + 3]),
                                          pk2bf(t[base + 4], t[base + 5]), pk2bf(t[base + 6], t[base + 7])});
}
__device__ __forceinline__ float max3f(float a, float b, float c) {  // (scores are finite or -inf: no NaN handling)
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float swap32max(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ float swap32sum(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}

// Per-lane LDS offsets of the fragment reads of a tile image (lane: hi = lane >> 5, c = lane & 31, a = lane >> 4,
// q = (lane & 15) >> 2, p = lane & 3), b = the tile's 32-row block:
//   k[4 b + s]:            row read, tile row 32 b + c, columns 16 s + 8 hi .. + 7
//   v[4 b + 2 db + part]:  transposed read, tile rows 32 b + 8 part + 4 hi + q (+ 16 sub: + 16 ROWB), columns
//                          32 db + 16 (a & 1) + 4 p .. + 3
struct Offs {
  int k[8], v[8];
  __device__ __forceinline__ void init(int lane) {
    const int c = lane & 31, hi = lane >> 5, a = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
    for (int s = 0; s < 8; ++s) k[s] = img_off(c, 2 * s + hi);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int part = 0; part < 2; ++part)
        v[2 * j + part] = img_off(8 * part + 4 * hi + q, 4 * j + 2 * (a & 1) + (p >> 1)) + 8 * (p & 1);
  }
};

// The DMA lane's source offset for image row r (LDS position pos of it): the chunk the swizzle puts there, taken from
// tile row r (chunks 0..7) or r + 32 (chunks 8..15) of a matrix whose rows are rowb bytes apart.
__device__ __forceinline__ unsigned dma_voff(int r, int pos, unsigned rowb) {
  const int ch = swz(r, pos);
  return (unsigned)(r + 32 * (ch >> 3)) * rowb + 16 * (ch & 7);
}

// Epilogue of a transposed [64 columns][32 rows] accumulator pair: lane (hi, c) holds columns 32 db + 8 m + 4 hi +
// {0..3} (registers 4 m .. 4 m + 3 of block db) of row c; one permlane32 swap per dword pair gives each half 8
// consecutive columns -> 4 x 16-B stores per lane. Every lane must call (the swaps).
__device__ __forceinline__ void store_rows(u16* row, const f32x16 (&a)[2], float s, bool ok) {
  const int hi = (threadIdx.x >> 5) & 1;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i0 = 8 * u;
      const unsigned ax = pk2bf(a[db][i0] * s, a[db][i0 + 1] * s);
      const unsigned ay = pk2bf(a[db][i0 + 2] * s, a[db][i0 + 3] * s);
      const unsigned bx = pk2bf(a[db][i0 + 4] * s, a[db][i0 + 5] * s);
      const unsigned by = pk2bf(a[db][i0 + 6] * s, a[db][i0 + 7] * s);
      const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
      const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
      if (ok) *(uint4*)(row + 32 * db + 16 * u + 8 * hi) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
}

// What the forward and the dQ kernel share: the workgroup's place, the key-tile range and the K / V tile DMA.
template <int HW>
struct QSide {
  static constexpr int PB = 4 / HW;
  int start, len, q0, lane, wave, hi, h, kvh, wq0, qi, nkt, lastkey, lim;
  long ld;
  unsigned rowb, voffk, voffv;
  bool qok;
  // false: the workgroup's queries are all past the sequence end
  __device__ __forceinline__ bool init(const int* __restrict__ cu, int nq, int nkv, int total, int causal) {
    const int b = blockIdx.y, qb = gridDim.z - 1 - blockIdx.z;  // the last (causally heaviest) block first
    start = cu[b];
    len = cu[b + 1] - start;
    SFT_DASSERT(start >= 0 && len >= 0 && start + len <= total);
    q0 = qb * 32 * PB;
    if (q0 >= len) return false;
    const int tid = threadIdx.x;
    lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    hi = lane >> 5;
    h = blockIdx.x * HW + wave % HW;
    kvh = (blockIdx.x * HW) / (nq / nkv);
    ld = (long)(nq + 2 * nkv) * D;
    rowb = (unsigned)ld * 2;
    wq0 = q0 + 32 * (wave / HW);
    qi = wq0 + (lane & 31);
    qok = qi < len;
    const int nkb = (len + 63) / 64;
    nkt = causal ? min((min(q0 + 32 * PB, len) - 1) / 64 + 1, nkb) : nkb;
    lastkey = causal ? min(wq0 + 31, len - 1) : len - 1;  // the wave's last visible key
    lim = causal ? min(len - 1, qi) : len - 1;            // this lane's last visible key
    // DMA lane (wave w, l) fills image rows 4 (w + 4 j) + (l >> 4), position l & 15 (the two rows share a swizzle)
    const int r0 = 4 * wave + (lane >> 4);
    voffk = dma_voff(r0, lane & 15, rowb);
    voffv = voffk + nkv * HROWB;
    return true;
  }
  // K and V of rows [0, len) of this kv head in one descriptor (V = K + nkv heads)
  __device__ __forceinline__ rsrc_t kv_rsrc(const u16* qkv, int nq) const {
    return make_rsrc(qkv + (long)start * ld + (nq + kvh) * D, (long)len * ld * 2 - (long)(nq + kvh) * HROWB);
  }
  // the 64-key tile at k0 into stage st: K image, then V image
  __device__ __forceinline__ void dma_tile(rsrc_t kv, char* st, int k0) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned so = (unsigned)(k0 + 16 * j) * rowb;
      bldsx4(kv, st + (wave + 4 * j) * 1024, voffk, so);
      bldsx4(kv, st + TB + (wave + 4 * j) * 1024, voffv, so);
    }
  }
  // 4 fragments (B operand, k = d) of this lane's row of a [len][row stride rb bytes] matrix; past the end: zero
  __device__ __forceinline__ void load_row(const u16* base, unsigned rb, bf16x8 (&f)[4]) const {
    const rsrc_t r = make_rsrc(base, (long)(len - 1) * rb + HROWB);
    const unsigned vo = (unsigned)qi * rb + 16 * hi;
#pragma unroll
    for (int st = 0; st < 4; ++st) f[st] = bload16(r, vo + 32 * st);
  }
};

// ============================================================================== forward
// grid (nq / HW, sequences, position blocks of 32 (4 / HW)); 256 threads
template <int HW>
__global__ __launch_bounds__(256, 3) void fwd_kernel(const u16* __restrict__ qkv, u16* __restrict__ out,
                                                     float* __restrict__ lse, const int* __restrict__ cu, int nq,
                                                     int nkv, int total, float sl2, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TB];  // two stages of (K image, V image)
  QSide<HW> w;
  if (!w.init(cu, nq, nkv, total, causal)) return;
  const int hi = w.hi;
  Offs off;
  off.init(w.lane);
  bf16x8 qf[4];
  w.load_row(qkv + (long)w.start * w.ld + w.h * D, w.rowb, qf);
  const rsrc_t kv = w.kv_rsrc(qkv, nq);
  w.dma_tile(kv, smem, 0);
  vm_drain();
  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
  float m = -1e30f, l = 0.f;  // l: this lane's partial row sum (its 16 keys of each 32-key block)
  __syncthreads();
  for (int kt = 0; kt < w.nkt; ++kt) {
    const int k0 = kt * 64;
    const bool pre = kt + 1 < w.nkt;
    const char* Ks = smem + (kt & 1) * 2 * TB;
    const char* Vs = Ks + TB;
    if (pre) w.dma_tile(kv, smem + ((kt + 1) & 1) * 2 * TB, k0 + 64);
    if (k0 <= w.lastkey) {                    // (wave-uniform) else: the whole tile is past the wave's diagonal
      const bool two = k0 + 32 <= w.lastkey;  // (wave-uniform) the second 32-key block has a visible key
      f32x16 s[2];
      s[0] = mfma32(lds_row(Ks, off.k[0]), qf[0], f32x16{});
#pragma unroll
      for (int st = 1; st < 4; ++st) s[0] = mfma32(lds_row(Ks, off.k[st]), qf[st], s[0]);
      if (two) {
        s[1] = mfma32(lds_row(Ks, off.k[4]), qf[0], f32x16{});
#pragma unroll
        for (int st = 1; st < 4; ++st) s[1] = mfma32(lds_row(Ks, off.k[4 + st]), qf[st], s[1]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[1][i] = -INFINITY;
      }
      if ((k0 + 64 > w.len) || (causal && k0 + 63 > w.wq0)) {  // only the diagonal and the last tiles
        const int rel = w.lim - k0 - 4 * hi;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int i = 0; i < 16; ++i) s[kb][i] = 32 * kb + (i & 3) + 8 * (i >> 2) > rel ? -INFINITY : s[kb][i];
      }
      float mx = max3f(s[0][0], s[0][1], s[0][2]);
#pragma unroll
      for (int i = 3; i < 15; i += 2) mx = max3f(mx, s[0][i], s[0][i + 1]);
      mx = max3f(mx, s[0][15], s[1][0]);
#pragma unroll
      for (int i = 1; i < 15; i += 2) mx = max3f(mx, s[1][i], s[1][i + 1]);
      mx = fmaxf(mx, s[1][15]);
      const float tmax = swap32max(mx) * sl2;
      if (__any(tmax > m + THR)) {  // deferred rescale: P stays <= 2^THR
        const float mnew = fmaxf(m, tmax);
        const float alpha = exp2f(m - mnew);
        l *= alpha;
        o[0] *= alpha;
        o[1] *= alpha;
        m = mnew;
      }
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const float p0 = exp2f(__builtin_fmaf(s[kb][i], sl2, -m));
          const float p1 = exp2f(__builtin_fmaf(s[kb][i + 1], sl2, -m));
          s[kb][i] = p0;
          s[kb][i + 1] = p1;
          acc0 += p0;
          acc1 += p1;
        }
      l += acc0 + acc1;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && !two) break;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const bf16x8 pb = pack_acc(s[kb], 8 * sub);
#pragma unroll
          for (int db = 0; db < 2; ++db)
            o[db] = mfma32(lds_tr2(Vs, off.v[4 * kb + 2 * db] + 16 * sub * ROWB,
                                   off.v[4 * kb + 2 * db + 1] + 16 * sub * ROWB), pb, o[db]);
        }
      }
    }
    if (pre) vm_drain();  // this lane's pieces of the next tile landed ...
    __syncthreads();      // ... and every lane's; every wave is done reading this stage
  }
  l = swap32sum(l);
  store_rows(out + (long)(w.start + w.qi) * nq * D + w.h * D, o, 1.f / l, w.qok);
  if (w.qok && hi == 0) lse[(long)w.h * total + w.start + w.qi] = (m + log2f(l)) * LN2;
}

// ============================================================================== backward
// delta[h][m] = sum_d dO[m, h, d] * O[m, h, d]: 8 lanes per row, each its 8 elements in order, then a xor tree
// (4, 2, 1)
__global__ __launch_bounds__(256) void delta_kernel(const u16* __restrict__ dout, const u16* __restrict__ out,
                                                    float* __restrict__ delta, int total, int nq) {
  const long rowid = blockIdx.x * 32L + (threadIdx.x >> 3);  // (m, h) flattened as m * nq + h
  const int sub = threadIdx.x & 7;
  float s = 0.f;
  const bool ok = rowid < (long)total * nq;
  if (ok) {
    const long base = rowid * D + sub * 8;
    float a[8], c[8];
    unpack8(*(const uint4*)(dout + base), a);
    unpack8(*(const uint4*)(out + base), c);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += a[i] * c[i];
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) s += __shfl_xor(s, o, 8);
  if (ok && sub == 0) {
    const long m = rowid / nq;
    const int h = (int)(rowid - m * nq);
    delta[(long)h * total + m] = s;
  }
}

// dQ: per 64-key tile S^T = K Q^T and dP^T = V dO^T (row reads of the K / V images, Q / dO fragments in registers),
// dS^T = P^T (dP^T - delta) with lse and delta one scalar per lane, dQ^T += K^T dS^T (transposed reads of the K image,
// dS^T from the accumulator). Per tile and wave: 24 MFMAs, 16 ds_read_b128 + 16 ds_read_b64_tr_b16.
template <int HW>
__global__ __launch_bounds__(256, 2) void bwd_dq_kernel(const u16* __restrict__ qkv, const u16* __restrict__ dout,
                                                        const float* __restrict__ lse,
                                                        const float* __restrict__ delta, const int* __restrict__ cu,
                                                        u16* __restrict__ dqkv, int nq, int nkv, int total, float sl2,
                                                        float scale, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TB];
  QSide<HW> w;
  if (!w.init(cu, nq, nkv, total, causal)) return;
  const int hi = w.hi;
  Offs off;
  off.init(w.lane);
  bf16x8 qf[4], df[4];
  w.load_row(qkv + (long)w.start * w.ld + w.h * D, w.rowb, qf);
  w.load_row(dout + (long)w.start * nq * D + w.h * D, (unsigned)nq * HROWB, df);
  // a row past the sequence end: Q = dO = 0, lse = delta = 0, so p = 1 and dS = 0
  const float lse2 = w.qok ? lse[(long)w.h * total + w.start + w.qi] * LOG2E : 0.f;
  const float dl = w.qok ? delta[(long)w.h * total + w.start + w.qi] : 0.f;
  const rsrc_t kv = w.kv_rsrc(qkv, nq);
  w.dma_tile(kv, smem, 0);
  vm_drain();
  f32x16 dq[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[db][i] = 0.f;
  __syncthreads();
  for (int kt = 0; kt < w.nkt; ++kt) {
    const int k0 = kt * 64;
    const bool pre = kt + 1 < w.nkt;
    const char* Ks = smem + (kt & 1) * 2 * TB;
    const char* Vs = Ks + TB;
    if (pre) w.dma_tile(kv, smem + ((kt + 1) & 1) * 2 * TB, k0 + 64);
    if (k0 <= w.lastkey) {
      const bool two = k0 + 32 <= w.lastkey;
      const bool need_mask = (k0 + 64 > w.len) || (causal && k0 + 63 > w.wq0);
      const int rel = w.lim - k0 - 4 * hi;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && !two) break;
        f32x16 s, dp;
        s = mfma32(lds_row(Ks, off.k[4 * kb]), qf[0], f32x16{});
        dp = mfma32(lds_row(Vs, off.k[4 * kb]), df[0], f32x16{});
#pragma unroll
        for (int st = 1; st < 4; ++st) {
          s = mfma32(lds_row(Ks, off.k[4 * kb + st]), qf[st], s);
          dp = mfma32(lds_row(Vs, off.k[4 * kb + st]), df[st], dp);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = exp2f(__builtin_fmaf(s[i], sl2, -lse2)) * (dp[i] - dl);
        if (need_mask) {  // a masked element's p may be inf: replaced, never multiplied
#pragma unroll
          for (int i = 0; i < 16; ++i) dp[i] = 32 * kb + (i & 3) + 8 * (i >> 2) > rel ? 0.f : dp[i];
        }
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const bf16x8 sb = pack_acc(dp, 8 * sub);
#pragma unroll
          for (int db = 0; db < 2; ++db)
            dq[db] = mfma32(lds_tr2(Ks, off.v[4 * kb + 2 * db] + 16 * sub * ROWB,
                                    off.v[4 * kb + 2 * db + 1] + 16 * sub * ROWB), sb, dq[db]);
        }
      }
    }
    if (pre) vm_drain();
    __syncthreads();
  }
  store_rows(dqkv + (long)(w.start + w.qi) * w.ld + w.h * D, dq, scale, w.qok);
}

// dK / dV. Per 64-query tile and wave (32 keys): 32 MFMAs, 16 ds_read_b128 + 32 ds_read_b64_tr_b16. The (head, query
// tile) pairs of a group run as one loop, so the Q / dO prefetch crosses from one head to the next.
// grid (nkv, sequences, key blocks of 64), 128 G threads: wave = 2 grp + kh
template <int G>
__global__ __launch_bounds__(128 * G, 2) void bwd_dkdv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ cu, u16* __restrict__ dqkv, int nq, int nkv, int total,
    float sl2, float scale, int causal) {
  constexpr int GB = 2 * TB + 2 * 64 * 4;  // per stage: Q, dO images + lse, delta of the tile's 64 queries
  __shared__ __attribute__((aligned(16))) char smem[G * 2 * GB];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wv >> 1, kh = wv & 1;
  const int gl = tid & 127, hi = lane >> 5;
  char* base = smem + grp * 2 * GB;
  const int kvh = blockIdx.x, b = blockIdx.y, kb = blockIdx.z;  // z = 0 first: the causally heaviest key blocks
  const int start = cu[b], len = cu[b + 1] - start;
  SFT_DASSERT(start >= 0 && len >= 0 && start + len <= total);
  const int k0 = kb * 64;
  if (k0 >= len) return;
  const int rep = nq / nkv, hpg = rep / G;
  const long ld = (long)(nq + 2 * nkv) * D, ldo = (long)nq * D;
  const unsigned rowb = (unsigned)ld * 2, rowo = (unsigned)ldo * 2;
  const int kw0 = k0 + 32 * kh, key = kw0 + (lane & 31);
  const bool kok = key < len;
  const int qt0 = causal ? kb : 0, nqt = (len + 63) / 64;
  const int niter = hpg * (nqt - qt0);
  Offs off;
  off.init(lane);
  // Q rows [0, len) of every head of the sequence (rows past it fall outside the range: zero), dO likewise
  const rsrc_t qr = make_rsrc(qkv + (long)start * ld, (long)(len - 1) * ld * 2 + (long)nq * HROWB);
  const rsrc_t orr = make_rsrc(dout + (long)start * ldo, (long)len * ldo * 2);
  // DMA: lane (wave kh, l) fills image rows 4 (kh + 2 j) + (l >> 4) = r0 + 8 j, position l & 15; rows r0 + 16 u and
  // r0 + 8 + 16 u have two swizzles: the even / odd pieces' lane offsets
  const int r0 = 4 * kh + (lane >> 4);
  const unsigned vq0 = dma_voff(r0, lane & 15, rowb), vq1 = dma_voff(r0 + 8, lane & 15, rowb);
  const unsigned vo0 = dma_voff(r0, lane & 15, rowo), vo1 = dma_voff(r0 + 8, lane & 15, rowo);
  auto dma_tile = [&](char* st, int h, int q0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bldsx4(qr, st + (kh + 2 * j) * 1024, (j & 1) ? vq1 : vq0, (unsigned)(q0 + 16 * (j >> 1)) * rowb + h * HROWB);
      bldsx4(orr, st + TB + (kh + 2 * j) * 1024, (j & 1) ? vo1 : vo0, (unsigned)(q0 + 16 * (j >> 1)) * rowo + h * HROWB);
    }
  };
  int h = kvh * rep + grp * hpg, qt = qt0;
  dma_tile(base, h, qt0 * 64);
  if (gl < 64) {
    const int q = qt0 * 64 + gl;
    float* Ls = (float*)(base + 2 * TB);
    Ls[gl] = q < len ? lse[(long)h * total + start + q] * LOG2E : 0.f;
    Ls[64 + gl] = q < len ? delta[(long)h * total + start + q] : 0.f;
  }
  // this lane's K and V rows (B operands of S = Q K^T and dP = dO V^T) in registers; keys past the end: zero
  bf16x8 kf[4], vf[4];
  {
    const rsrc_t kr = make_rsrc(qkv + (long)start * ld + (nq + kvh) * D, (long)(len - 1) * ld * 2 + (long)(nkv + 1) * HROWB);
    const unsigned vo = (unsigned)key * rowb + 16 * hi;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      kf[st] = bload16(kr, vo + 32 * st);
      vf[st] = bload16(kr, vo + nkv * HROWB + 32 * st);
    }
  }
  vm_drain();
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[db][i] = dv[db][i] = 0.f;
  __syncthreads();
  for (int it = 0; it < niter; ++it) {
    const int q0 = qt * 64;
    const bool pre = it + 1 < niter;
    int hn = h, qtn = qt + 1;
    if (qtn == nqt) {
      qtn = qt0;
      ++hn;
    }
    const char* Qs = base + (it & 1) * GB;
    const char* Os = Qs + TB;
    const float* Ls = (const float*)(Qs + 2 * TB);
    char* nxt = base + ((it + 1) & 1) * GB;
    float pl = 0.f, pd = 0.f;
    if (pre) {
      dma_tile(nxt, hn, qtn * 64);
      if (gl < 64 && qtn * 64 + gl < len) {
        pl = lse[(long)hn * total + start + qtn * 64 + gl];
        pd = delta[(long)hn * total + start + qtn * 64 + gl];
      }
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16 s, dp;
      s = mfma32(lds_row(Qs, off.k[4 * qb]), kf[0], f32x16{});
      dp = mfma32(lds_row(Os, off.k[4 * qb]), vf[0], f32x16{});
#pragma unroll
      for (int st = 1; st < 4; ++st) {
        s = mfma32(lds_row(Qs, off.k[4 * qb + st]), kf[st], s);
        dp = mfma32(lds_row(Os, off.k[4 * qb + st]), vf[st], dp);
      }
      // register 4 m + t is query q0 + 32 qb + 4 hi + o, o = 8 m + t; visible iff lo <= o <= hq
      const int qbase = q0 + 32 * qb + 4 * hi;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float4 L4 = *(const float4*)(Ls + 32 * qb + 8 * m + 4 * hi);
        const float4 D4 = *(const float4*)(Ls + 64 + 32 * qb + 8 * m + 4 * hi);
        const float L[4] = {L4.x, L4.y, L4.z, L4.w}, Dd[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int i = 4 * m + t;
          const float p = exp2f(__builtin_fmaf(s[i], sl2, -L[t]));
          dp[i] = p * (dp[i] - Dd[t]);
          s[i] = p;
        }
      }
      // (wave-uniform branch) only the diagonal and the sequence-end tiles; a masked p may be inf: replaced
      if ((q0 + 32 * qb + 31 >= len) || (causal && kw0 + 31 > q0 + 32 * qb)) {
        const int lo = (causal ? key : 0) - qbase, hq = len - 1 - qbase;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int o = 8 * (i >> 2) + (i & 3);
          if (o < lo || o > hq) s[i] = dp[i] = 0.f;
        }
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const bf16x8 pb = pack_acc(s, 8 * sub), sb = pack_acc(dp, 8 * sub);
        const int ko = 16 * sub * ROWB;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dv[db] = mfma32(lds_tr2(Os, off.v[4 * qb + 2 * db] + ko, off.v[4 * qb + 2 * db + 1] + ko), pb, dv[db]);
          dk[db] = mfma32(lds_tr2(Qs, off.v[4 * qb + 2 * db] + ko, off.v[4 * qb + 2 * db + 1] + ko), sb, dk[db]);
        }
      }
    }
    if (pre && gl < 64) {  // the next stage's lse / delta (that stage's last reads ended at the previous barrier)
      float* Ln = (float*)(nxt + 2 * TB);
      Ln[gl] = pl * LOG2E;
      Ln[64 + gl] = pd;
    }
    if (pre) vm_drain();  // this lane's pieces of the next tile landed ...
    __syncthreads();      // ... and every lane's; every wave is done reading this stage
    h = hn;
    qt = qtn;
  }
  if constexpr (G == 2) {  // group 1 hands its dK / dV partial sums to group 0 through the (now idle) stages
    float4* xk = (float4*)smem;
    float4* xv = xk + 2 * 8 * 64;
    if (grp == 1) {
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int ix = (kh * 8 + 4 * db + v) * 64 + lane;
          xk[ix] = make_float4(dk[db][4 * v], dk[db][4 * v + 1], dk[db][4 * v + 2], dk[db][4 * v + 3]);
          xv[ix] = make_float4(dv[db][4 * v], dv[db][4 * v + 1], dv[db][4 * v + 2], dv[db][4 * v + 3]);
        }
    }
    __syncthreads();
    if (grp == 1) return;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int ix = (kh * 8 + 4 * db + v) * 64 + lane;
        const float4 a = xk[ix], c = xv[ix];
        dk[db][4 * v] += a.x;
        dk[db][4 * v + 1] += a.y;
        dk[db][4 * v + 2] += a.z;
        dk[db][4 * v + 3] += a.w;
        dv[db][4 * v] += c.x;
        dv[db][4 * v + 1] += c.y;
        dv[db][4 * v + 2] += c.z;
        dv[db][4 * v + 3] += c.w;
      }
  }
  store_rows(dqkv + (long)(start + key) * ld + (nq + kvh) * D, dk, scale, kok);
  store_rows(dqkv + (long)(start + key) * ld + (nq + nkv + kvh) * D, dv, 1.f, kok);
}

// ------------------------------------------------------------------------------ host
// The kernels' 32-bit buffer offsets: the rows of one sequence (plus the tile a prefetch may reach past its end)
static void check_span(int nq, int nkv, int max_seqlen) {
  SFT_CHECK(((long)max_seqlen + 128) * (nq + 2 * nkv) * HROWB < (1L << 32),
            "flash attention (head_dim 64): a sequence of ", max_seqlen, " tokens spans 4 GiB of qkv or more");
}

void launch_fwd(const u16* qkv, u16* out, float* lse, const int* cu, int nq, int nkv, int total, int nseq,
                int max_seqlen, float sl2, int causal, hipStream_t st) {
  check_span(nq, nkv, max_seqlen);
  SFT_TRACE("attn.fwd_d64");
  const int rep = nq / nkv, hw = rep % 4 == 0 ? 4 : rep % 2 == 0 ? 2 : 1, span = 32 * (4 / hw);
  dim3 g(nq / hw, nseq, (max_seqlen + span - 1) / span);
  if (hw == 4) fwd_kernel<4><<<g, 256, 0, st>>>(qkv, out, lse, cu, nq, nkv, total, sl2, causal);
  else if (hw == 2) fwd_kernel<2><<<g, 256, 0, st>>>(qkv, out, lse, cu, nq, nkv, total, sl2, causal);
  else fwd_kernel<1><<<g, 256, 0, st>>>(qkv, out, lse, cu, nq, nkv, total, sl2, causal);
  SFT_LAUNCH_CHECK();
}

void launch_delta(const u16* dout, const u16* out, float* delta, int total, int nq, hipStream_t st) {
  SFT_TRACE("attn.delta_d64");
  const long rows = (long)total * nq;
  delta_kernel<<<(rows + 31) / 32, 256, 0, st>>>(dout, out, delta, total, nq);
  SFT_LAUNCH_CHECK();
}

void launch_bwd(const u16* qkv, const u16* dout, const float* lse, const float* delta, const int* cu, u16* dqkv, int nq,
                int nkv, int total, int nseq, int max_seqlen, float sl2, float scale, int causal, hipStream_t st) {
  check_span(nq, nkv, max_seqlen);
  const int rep = nq / nkv;
  SFT_TRACE("attn.dkdv_d64");
  dim3 gk(nkv, nseq, (max_seqlen + 63) / 64);
  if (rep % 2 == 0)
    bwd_dkdv_kernel<2><<<gk, 256, 0, st>>>(qkv, dout, lse, delta, cu, dqkv, nq, nkv, total, sl2, scale, causal);
  else
    bwd_dkdv_kernel<1><<<gk, 128, 0, st>>>(qkv, dout, lse, delta, cu, dqkv, nq, nkv, total, sl2, scale, causal);
  SFT_LAUNCH_CHECK();
  SFT_TRACE("attn.dq_d64");
  const int hw = rep % 4 == 0 ? 4 : rep % 2 == 0 ? 2 : 1, span = 32 * (4 / hw);
  dim3 gq(nq / hw, nseq, (max_seqlen + span - 1) / span);
  if (hw == 4) bwd_dq_kernel<4><<<gq, 256, 0, st>>>(qkv, dout, lse, delta, cu, dqkv, nq, nkv, total, sl2, scale, causal);
  else if (hw == 2) bwd_dq_kernel<2><<<gq, 256, 0, st>>>(qkv, dout, lse, delta, cu, dqkv, nq, nkv, total, sl2, scale, causal);
  else bwd_dq_kernel<1><<<gq, 256, 0, st>>>(qkv, dout, lse, delta, cu, dqkv, nq, nkv, total, sl2, scale, causal);
  SFT_LAUNCH_CHECK();
}

}  // namespace attn64
}  // namespace sftamd
