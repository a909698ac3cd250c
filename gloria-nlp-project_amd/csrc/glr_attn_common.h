// Device helpers and the parameter block shared by the text-encoder self-attention kernels: glr_attn.hip (L <= 128, a head
// is one score tile) and glr_attn_long.hip (L <= 512, 128-token blocks streamed through LDS).
#pragma once
#include "glr_common.h"

namespace {

constexpr int AT_NT = 256;
constexpr int AT_RP = 144;            // bytes per row of a row-major [token][64] LDS operand (128 + 16: bank spread)
constexpr int AT_SP = 272;            // bytes per row of a wave's score / staging slab: 128 keys + 16
constexpr float AT_LOG2E = 1.4426950408889634f;

struct AttnParams {
  const unsigned short* q; const unsigned short* k; const unsigned short* v;   // [B, L, ld]
  const unsigned char* key_mask;    // [B, L] nonzero = attend; NULL = all
  int B, nh, L, ld, ld_o;           // row strides (elements) of q / k / v / dq / dk / dv and of o / d_o
  float scale, p_drop;
  unsigned seed_lo, seed_hi, off_lo, off_hi;
  const unsigned long long* rng;   // NULL, or device cell {seed, offset base}: key = (rng[0], rng[1] + offset) (hipGraph replays)
  unsigned short* o;                // fwd out / bwd in
  float* lse;                       // [B * nh, 128]
  unsigned* keep;                   // [B * nh, 128, 4] keep bits: key 32 j + i of query row r = bit i of word (r, j)
  const unsigned short* d_o;        // bwd
  unsigned short* dq; unsigned short* dk; unsigned short* dv;
  int tp;                           // bytes per row of a token-contiguous LDS operand: max(2 * ceil16(L) + 16, 144)
  const int* row_start;             // NULL, or [B + 1]: sentence b = rows [row_start[b], row_start[b + 1]) of a packed [T, ld]
                                    // tensor (no pad rows, no key mask); L is then the longest sentence of the batch
};

// first row and token count of sentence b: the padded [B, L, ld] layout, or the packed one through row_start (the count is
// held to the host's maximum, which sized tp and the LDS)
__device__ __forceinline__ void attn_rows(const AttnParams& p, int b, size_t& row_base, int& L) {
  L = p.L;
  row_base = (size_t)b * L;
  if (p.row_start != nullptr) {
    const int r0 = p.row_start[b], n = p.row_start[b + 1] - r0;
    row_base = (size_t)r0;
    L = n < p.L ? n : p.L;
  }
}

// dropout bits: a counter-based hash (two rounds of a 32-bit multiply-xorshift mixer, keyed by seed and offset) of the
// score's position - 16 bits per score.  (Philox4x32-10 cost 40 quarter-rate integer multiplies per 8 scores here.)
__device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned hash32(unsigned ctr, unsigned k0, unsigned k1) { return mix32(mix32(ctr ^ k0) + k1); }

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// reductions over the 32 lanes of a lane half (every lane ends up with the result)
__device__ __forceinline__ float half_max(float v) {
  v = fmaxf(v, dpp<0xB1>(v));       // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp<0x4E>(v));       // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp<0x141>(v));      // row_half_mirror
  v = fmaxf(v, dpp<0x140>(v));      // row_mirror
  return fmaxf(v, __shfl_xor(v, 16, 64));
}
__device__ __forceinline__ float half_sum(float v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x141>(v);
  v += dpp<0x140>(v);
  return v + __shfl_xor(v, 16, 64);
}

__device__ __forceinline__ bf16x8 ldf(const unsigned char* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); }
__device__ __forceinline__ void mma(const bf16x8& a, const bf16x8& b, f32x16& c) { c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int q = 0; q < 16; ++q) a[q] = 0.f;
}
// accumulator register q of a 32x32 block -> row inside the block (column = lane & 31)
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// A [L x 64] bf16 head tile (row stride ld elements) is moved in two steps so that ALL global loads of a workgroup are
// in flight together (a load -> LDS-store loop per operand exposes the full memory latency once per iteration: with one
// workgroup per CU that was 12 (forward) / 28 (backward) serial round trips and most of the kernel time):
// item i = tid + 256 t, t = 0..3: token row i & 127, 16-byte piece i >> 7 (rows >= L read as zero): the lanes of a wave
// hold consecutive tokens of one piece, so the transposed LDS stores below are contiguous 2-byte runs (conflict-free).
__device__ __forceinline__ void tile_load(const unsigned short* g, int ld, int L, uint4 (&r)[4], int tid) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + AT_NT * t, row = i & 127, pc = i >> 7;
    r[t] = make_uint4(0u, 0u, 0u, 0u);
    if (row < L) r[t] = *reinterpret_cast<const uint4*>(g + (size_t)row * ld + pc * 8);
  }
}
// -> LDS row-major, 128 rows of AT_RP bytes
__device__ __forceinline__ void tile_store_rows(const uint4 (&r)[4], unsigned char* dst, int tid) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + AT_NT * t, row = i & 127, pc = i >> 7;
    *reinterpret_cast<uint4*>(dst + row * AT_RP + pc * 16) = r[t];
  }
}
// -> LDS transposed: dst[d][token], tp bytes per row, tokens [L, ceil16(L)) zero
__device__ __forceinline__ void tile_store_transposed(const uint4 (&r)[4], int lk, unsigned char* dst, int tp, int tid) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + AT_NT * t, row = i & 127, pc = i >> 7;
    if (row < lk) {
      const unsigned w[4] = {r[t].x, r[t].y, r[t].z, r[t].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *reinterpret_cast<unsigned short*>(dst + (pc * 8 + 2 * e) * tp + row * 2) = (unsigned short)(w[e] & 0xffffu);
        *reinterpret_cast<unsigned short*>(dst + (pc * 8 + 2 * e + 1) * tp + row * 2) = (unsigned short)(w[e] >> 16);
      }
    }
  }
}
__device__ __forceinline__ float dot8(const uint4 a, const uint4 c) {
  const unsigned aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
  float d = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    d = __builtin_fmaf(__uint_as_float(aw[e] << 16), __uint_as_float(cw[e] << 16), d);
    d = __builtin_fmaf(__uint_as_float(aw[e] & 0xffff0000u), __uint_as_float(cw[e] & 0xffff0000u), d);
  }
  return d;
}
// acc[j] = A_rows(32 rows at arow0) . B_rows(block j)^T over 64 features, both row-major AT_RP operands
__device__ __forceinline__ void gemm_rows64(f32x16 (&acc)[4], const unsigned char* A, int arow0, const unsigned char* Bm, int nblk,
                                            int l31, int h) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const bf16x8 fa = ldf(A + (arow0 + l31) * AT_RP + ks * 32 + h * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nblk) mma(fa, ldf(Bm + (32 * j + l31) * AT_RP + ks * 32 + h * 16), acc[j]);
  }
}
// out[c] = slab_rows(32) . Bt_rows(block c)^T over kt 16-token steps, both token-contiguous operands (tp bytes per row)
__device__ __forceinline__ void gemm_tokens(f32x16 (&out)[2], const unsigned char* slab, const unsigned char* Bt, int tp, int kt,
                                            int l31, int h) {
  for (int ks = 0; ks < kt; ++ks) {
    const bf16x8 fa = ldf(slab + l31 * AT_SP + ks * 32 + h * 16);
#pragma unroll
    for (int c = 0; c < 2; ++c) mma(fa, ldf(Bt + (32 * c + l31) * tp + ks * 32 + h * 16), out[c]);
  }
}
// a wave's 32 x 64 fp32 result -> bf16 rows of a [B, L, ld] tensor, through the wave's slab (16-byte stores)
__device__ __forceinline__ void store_rows(const f32x16 (&out)[2], unsigned char* slab, int tp, unsigned short* g, int ld, int row0, int L,
                                           int lane, int l31, int h) {
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < 16; ++q)
      *reinterpret_cast<unsigned short*>(slab + acc_row(q, h) * AT_SP + (32 * c + l31) * 2) = f2bf(out[c][q]);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = lane + 64 * t, row = i >> 3, pc = i & 7;
    if (row0 + row < L)
      *reinterpret_cast<uint4*>(g + (size_t)(row0 + row) * ld + pc * 8) = *reinterpret_cast<const uint4*>(slab + row * AT_SP + pc * 16);
  }
}

// the wave's own 32 rows - the A operand of its score products - go straight from global memory into MFMA fragments
__device__ __forceinline__ void frag_rows_load(const unsigned short* g, int ld, int row, int L, int h, bf16x8 (&f)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < L) v = *reinterpret_cast<const uint4*>(g + (size_t)row * ld + ks * 16 + h * 8);
    f[ks] = __builtin_bit_cast(bf16x8, v);
  }
}
__device__ __forceinline__ void gemm_frag64(f32x16 (&acc)[4], const bf16x8 (&fa)[4], const unsigned char* Bm, int nblk, int l31, int h) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nblk) mma(fa[ks], ldf(Bm + (32 * j + l31) * AT_RP + ks * 32 + h * 16), acc[j]);
}

// key of the counter hash: (seed, offset), or (rng[0], rng[1] + offset) read from the device cell
__device__ __forceinline__ void hash_key(const AttnParams& p, unsigned& hk0, unsigned& hk1) {
  unsigned sd_lo = p.seed_lo, sd_hi = p.seed_hi, of_lo = p.off_lo, of_hi = p.off_hi;
  if (p.rng != nullptr) {
    const unsigned long long s = p.rng[0], o = p.rng[1] + (((unsigned long long)p.off_hi << 32) | p.off_lo);
    sd_lo = (unsigned)s; sd_hi = (unsigned)(s >> 32); of_lo = (unsigned)o; of_hi = (unsigned)(o >> 32);
  }
  hk0 = sd_lo ^ (of_lo * 0x9E3779B9u); hk1 = sd_hi ^ (of_hi * 0x85EBCA6Bu) ^ 0xC2B2AE35u;
}

// bytes per row of the token-contiguous (transposed) LDS operands
inline int attn_tp(int L) { return 2 * ((L + 15) & ~15) + 16; }

inline int attn_fill(AttnParams& p, const void* q, const void* k, const void* v, const unsigned char* key_mask, int B, int nh, int L, int ld,
                     int ld_o, float scale, float p_drop, unsigned long long seed, unsigned long long offset, int max_L) {
  if (!q || !k || !v || B <= 0 || nh <= 0 || L <= 0 || L > max_L || ld < nh * 64 || ld % 8 != 0 || ld_o < nh * 64 || ld_o % 8 != 0)
    return GLR_EINVAL;
  if (p_drop < 0.f || p_drop >= 1.f) return GLR_EINVAL;
  p.q = (const unsigned short*)q; p.k = (const unsigned short*)k; p.v = (const unsigned short*)v; p.key_mask = key_mask;
  p.B = B; p.nh = nh; p.L = L; p.ld = ld; p.ld_o = ld_o; p.scale = scale; p.p_drop = p_drop;
  p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.off_lo = (unsigned)offset; p.off_hi = (unsigned)(offset >> 32);
  p.rng = nullptr; p.row_start = nullptr;
  p.o = nullptr; p.lse = nullptr; p.keep = nullptr; p.d_o = nullptr; p.dq = p.dk = p.dv = nullptr;
  p.tp = attn_tp(L < 128 ? L : 128);
  return GLR_OK;
}

}  // namespace
