// Self-attention of the BERT text encoder for short sequences (L <= 128 tokens, head size 64), forward and backward:
// softmax(Q K^T / sqrt(d) + key mask) -> dropout -> . V, one workgroup per (sentence, head), everything in LDS.
// Replaces BertSelfAttention's matmul / softmax / dropout / matmul (transformers' modeling_bert as built by
// /root/reference/gloria/models/text_model.py:18-20; 97 tokens per caption in imagenome_pretrain_config.yaml).
//
// Why not the library kernel: at 97 tokens the flash-attention kernels torch dispatches take 95 us forward and 390 us
// backward per layer for 7 + 18 GFLOP - they tile for long sequences.  Here a head is ONE 128 x 128 score tile:
//   forward   Q, K row-major and V transposed in LDS (53 KB: three workgroups per CU); wave w owns query rows
//             32w..32w+31: S (16 MFMA 32x32x16),
//             row softmax across the 32 lanes of a lane half (DPP butterflies), dropout, P -> the wave's LDS slab,
//             O = P V (2 x L/16 MFMA).  Saves lse per row and the dropout keep bits (1 bit per score).
//   backward  two passes, each a kernel of its own (56 / 72 KB of LDS: two workgroups per CU), waves independent after
//             the cooperative load, no atomics, no cross-wave reductions:
//             pass Q (wave owns 32 queries): S, dP = dO V^T, dS -> slab, dQ = dS K;
//             pass K (wave owns 32 keys):    S^T = K Q^T, dP^T = V dO^T (the same products with the operands
//             swapped land key-major in the accumulators), P^T -> slab, dV = P^T dO, dS^T -> slab, dK = dS^T Q.
//             Every product is an "A . B^T" of two k-contiguous operands: the wave's own rows come straight from
//             global memory as MFMA fragments, the other side sits in LDS; the three operands that are contracted
//             over tokens (K for dQ, dO for dV, Q for dK) get a transposed LDS copy at load time.
// Tensors are the [B, L, n_heads * 64] outputs of the query / key / value Linears read in place (row stride = hidden
// size); O and the gradients are written in the same layout, so no permute / contiguous copies exist around the op.
// Dropout bits: a keyed counter hash of (head, query row, key): a pure function of (seed, offset, position); the
// backward reads the stored bits and never runs the generator.
#include "glr_attn_common.h"

namespace {

__global__ void __launch_bounds__(AT_NT) k_attn_fwd(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int bh = blockIdx.x, b = bh / p.nh, hd = bh % p.nh;
  int L; size_t row_base;
  attn_rows(p, b, row_base, L);
  const int tp = p.tp, lk = (L + 15) & ~15, kt = lk >> 4, nkb = (L + 31) >> 5;
  unsigned char* Qs = smem;
  unsigned char* Ks = Qs + 128 * AT_RP;
  unsigned char* Vt = Ks + 128 * AT_RP;
  unsigned char* Ps = smem;                      // the P slabs take the place of Q / K once every wave has its scores
  float* kb = reinterpret_cast<float*>(Vt + 64 * tp);
  const size_t base = row_base * p.ld + (size_t)hd * 64;
  {
    uint4 rq[4], rk[4], rv[4];
    tile_load(p.q + base, p.ld, L, rq, tid);
    tile_load(p.k + base, p.ld, L, rk, tid);
    tile_load(p.v + base, p.ld, L, rv, tid);
    tile_store_rows(rq, Qs, tid);
    tile_store_rows(rk, Ks, tid);
    tile_store_transposed(rv, lk, Vt, tp, tid);
  }
  if (tid < 128) kb[tid] = (tid < L && (p.key_mask == nullptr || p.key_mask[(size_t)b * L + tid] != 0)) ? 0.f : -INFINITY;
  __syncthreads();
  const int row0 = 32 * wave;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zero16(acc[j]);
  if (row0 < L) gemm_rows64(acc, Qs, row0, Ks, nkb, l31, h);
  __syncthreads();                              // Q / K are dead: their space becomes the P slabs
  if (row0 >= L) return;                        // no barrier below: a wave without query rows is done
  float kbv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kbv[j] = kb[32 * j + l31];
  const bool drop = p.p_drop > 0.f;
  const unsigned thr16 = drop ? (unsigned)(p.p_drop * 65536.f + 0.5f) : 0u;
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  const float sl = p.scale * AT_LOG2E;
  unsigned char* slab = Ps + wave * 32 * AT_SP;
  unsigned mw0 = 0u, mw1 = 0u;
  unsigned hk0, hk1;
  hash_key(p, hk0, hk1);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int r = acc_row(q, h);
    float v[4], m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = __builtin_fmaf(acc[j][q], sl, kbv[j]); m = fmaxf(m, v[j]); }
    m = half_max(m);
    const float ms = m == -INFINITY ? 0.f : m;                     // a sentence with every key masked: all-zero row
    float e[4], s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { e[j] = __builtin_amdgcn_exp2f(v[j] - ms); s += e[j]; }
    s = half_sum(s);
    const float inv = s > 0.f ? 1.f / s : 0.f;
    if (l31 == 0) p.lse[(size_t)bh * 128 + row0 + r] = (ms + __builtin_amdgcn_logf(fmaxf(s, 1e-37f))) * (1.f / AT_LOG2E);
    unsigned r01 = 0u, r23 = 0u;
    if (drop) {
      const unsigned ctr = (((unsigned)bh * 128u + (unsigned)(row0 + r)) * 32u + (unsigned)l31) * 2u;
      r01 = hash32(ctr, hk0, hk1);
      r23 = hash32(ctr + 1u, hk0, hk1);
    }
    const unsigned r16[4] = {r01 & 0xffffu, r01 >> 16, r23 & 0xffffu, r23 >> 16};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool keepb = !drop || r16[j] >= thr16;
      if (drop) {
        const unsigned long long word = __ballot(keepb);
        if (lane == q * 4 + j) { mw0 = (unsigned)word; mw1 = (unsigned)(word >> 32); }
      }
      const float pd = keepb ? e[j] * inv * inv_keep : 0.f;
      *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(pd);
    }
  }
  if (drop) {
    const int q = lane >> 2, j = lane & 3;
    const int r0 = row0 + acc_row(q, 0);
    p.keep[((size_t)bh * 128 + r0) * 4 + j] = mw0;
    p.keep[((size_t)bh * 128 + r0 + 4) * 4 + j] = mw1;
  }
  f32x16 out[2];
  zero16(out[0]); zero16(out[1]);
  gemm_tokens(out, slab, Vt, tp, kt, l31, h);
  store_rows(out, slab, tp, p.o + row_base * p.ld_o + (size_t)hd * 64, p.ld_o, row0, L, lane, l31, h);
}

// ---- backward, split by pass so that two workgroups fit a CU (56 / 72 KB of LDS instead of 155 KB in one kernel:
// at one workgroup of four waves per CU every latency of the long dependent chains is exposed).  The wave's own 32
// rows - the A operand of its score products - go straight from global memory into MFMA fragments; the B operands
// are staged in LDS, and their space becomes the wave slabs once every wave has its two score tiles.
// pass Q: workgroup = (sentence, head), wave = 32 query rows: S, dP = dO V^T, dS -> slab, dQ = dS K
__global__ void __launch_bounds__(AT_NT, 2) k_attn_bwd_q(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int bh = blockIdx.x, b = bh / p.nh, hd = bh % p.nh;
  int L; size_t row_base;
  attn_rows(p, b, row_base, L);
  const int tp = p.tp, lk = (L + 15) & ~15, kt = lk >> 4, nkb = (L + 31) >> 5;
  unsigned char* Ks = smem;
  unsigned char* Vs = Ks + 128 * AT_RP;
  unsigned char* Kt = Vs + 128 * AT_RP;
  unsigned char* Ps = smem;                      // slabs take the place of K / V
  float* kb = reinterpret_cast<float*>(Kt + 64 * tp);
  float* lse = kb + 128;
  float* delta = lse + 128;                                       // [128], rows of wave w written by wave w
  unsigned* keep = reinterpret_cast<unsigned*>(delta + 128);      // [128][4]
  const size_t base = row_base * p.ld + (size_t)hd * 64, base_o = row_base * p.ld_o + (size_t)hd * 64;
  const bool drop = p.p_drop > 0.f;
  const int row0 = 32 * wave;
  const bool active = row0 < L;
  bf16x8 fq[4], fg[4];
  {
    uint4 rk[4], rv[4];
    bf16x8 fo[4];
    tile_load(p.k + base, p.ld, L, rk, tid);
    tile_load(p.v + base, p.ld, L, rv, tid);
    frag_rows_load(p.q + base, p.ld, row0 + l31, L, h, fq);
    frag_rows_load(p.d_o + base_o, p.ld_o, row0 + l31, L, h, fg);
    frag_rows_load(p.o + base_o, p.ld_o, row0 + l31, L, h, fo);
    if (tid < 128) {
      kb[tid] = (tid < L && (p.key_mask == nullptr || p.key_mask[(size_t)b * L + tid] != 0)) ? 0.f : -INFINITY;
      lse[tid] = tid < L ? p.lse[(size_t)bh * 128 + tid] * AT_LOG2E : 0.f;
    }
    for (int i = tid; i < 512; i += AT_NT) keep[i] = (drop && (i >> 2) < L) ? p.keep[(size_t)bh * 512 + i] : 0xffffffffu;
    tile_store_rows(rk, Ks, tid);
    tile_store_rows(rv, Vs, tid);
    tile_store_transposed(rk, lk, Kt, tp, tid);
    // delta[row] = <dO[row], O[row]>: a lane holds half of its row (the k pieces of its lane half)
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) d += dot8(__builtin_bit_cast(uint4, fg[ks]), __builtin_bit_cast(uint4, fo[ks]));
    d += __shfl_xor(d, 32, 64);
    if (h == 0) delta[row0 + l31] = d;
  }
  __syncthreads();
  f32x16 acc[4], acc2[4], out[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) { zero16(acc[j]); zero16(acc2[j]); }
  if (active) {
    gemm_frag64(acc, fq, Ks, nkb, l31, h);                 // S
    gemm_frag64(acc2, fg, Vs, nkb, l31, h);                // dP (before the dropout scaling) = dO V^T
  }
  __syncthreads();                              // K / V rows are dead: their space becomes the slabs
  if (!active) return;                          // no barrier below
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  const float sl = p.scale * AT_LOG2E;
  unsigned char* slab = Ps + wave * 32 * AT_SP;
  {
    float kbv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kbv[j] = kb[32 * j + l31];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = acc_row(q, h);
      const float lr = lse[row0 + r], dl = delta[row0 + r];
      const uint4 kw = *reinterpret_cast<const uint4*>(keep + (row0 + r) * 4);
      const unsigned kwj[4] = {kw.x, kw.y, kw.z, kw.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], sl, kbv[j]) - lr);
        const float dp = ((kwj[j] >> l31) & 1u) ? acc2[j][q] * inv_keep : 0.f;
        *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(pr * (dp - dl) * p.scale);
      }
    }
  }
  zero16(out[0]); zero16(out[1]);
  gemm_tokens(out, slab, Kt, tp, kt, l31, h);             // dQ = dS K
  store_rows(out, slab, tp, p.dq + base, p.ld, row0, L, lane, l31, h);
}

// pass K: wave = 32 key rows: S^T = K Q^T, dP^T = V dO^T, P^T -> slab, dV = P^T dO, dS^T -> slab, dK = dS^T Q
__global__ void __launch_bounds__(AT_NT, 2) k_attn_bwd_kv(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int bh = blockIdx.x, b = bh / p.nh, hd = bh % p.nh;
  int L; size_t row_base;
  attn_rows(p, b, row_base, L);
  const int tp = p.tp, lk = (L + 15) & ~15, kt = lk >> 4, nkb = (L + 31) >> 5;
  unsigned char* Qs = smem;
  unsigned char* Gs = Qs + 128 * AT_RP;          // dO
  unsigned char* Qt = Gs + 128 * AT_RP;
  unsigned char* Gt = Qt + 64 * tp;
  unsigned char* Ps = smem;                      // slabs take the place of Q / dO rows
  float* kb = reinterpret_cast<float*>(Gt + 64 * tp);
  float* lse = kb + 128;
  float* delta = lse + 128;                                       // [2][128] partial sums (the two thread halves)
  unsigned* keep = reinterpret_cast<unsigned*>(delta + 256);      // [128][4]
  const size_t base = row_base * p.ld + (size_t)hd * 64, base_o = row_base * p.ld_o + (size_t)hd * 64;
  const bool drop = p.p_drop > 0.f;
  const int row0 = 32 * wave;
  const bool active = row0 < L;
  bf16x8 fk[4], fv[4];
  {
    uint4 rq[4], rg[4], ro[4];
    tile_load(p.q + base, p.ld, L, rq, tid);
    tile_load(p.d_o + base_o, p.ld_o, L, rg, tid);
    tile_load(p.o + base_o, p.ld_o, L, ro, tid);
    frag_rows_load(p.k + base, p.ld, row0 + l31, L, h, fk);
    frag_rows_load(p.v + base, p.ld, row0 + l31, L, h, fv);
    if (tid < 128) {
      kb[tid] = (tid < L && (p.key_mask == nullptr || p.key_mask[(size_t)b * L + tid] != 0)) ? 0.f : -INFINITY;
      lse[tid] = tid < L ? p.lse[(size_t)bh * 128 + tid] * AT_LOG2E : 0.f;
    }
    for (int i = tid; i < 512; i += AT_NT) keep[i] = (drop && (i >> 2) < L) ? p.keep[(size_t)bh * 512 + i] : 0xffffffffu;
    tile_store_rows(rq, Qs, tid);
    tile_store_rows(rg, Gs, tid);
    tile_store_transposed(rq, lk, Qt, tp, tid);
    tile_store_transposed(rg, lk, Gt, tp, tid);
    delta[tid] = (dot8(rg[0], ro[0]) + dot8(rg[1], ro[1])) + (dot8(rg[2], ro[2]) + dot8(rg[3], ro[3]));
  }
  __syncthreads();
  f32x16 acc[4], acc2[4], out[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) { zero16(acc[j]); zero16(acc2[j]); }
  float lq[4], dq_[4], kbk16[16];
  unsigned kwq[4];
  if (active) {
    gemm_frag64(acc, fk, Qs, nkb, l31, h);                 // S^T
    gemm_frag64(acc2, fv, Gs, nkb, l31, h);                // dP^T = V dO^T
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lq[j] = lse[32 * j + l31];
    dq_[j] = delta[32 * j + l31] + delta[128 + 32 * j + l31];
    kwq[j] = keep[(32 * j + l31) * 4 + wave];            // keys of this wave's block, of query 32 j + l31
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) kbk16[q] = kb[row0 + acc_row(q, h)];
  __syncthreads();                              // Q / dO rows are dead: their space becomes the slabs
  if (!active) return;                          // no barrier below
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  const float sl = p.scale * AT_LOG2E;
  unsigned char* slab = Ps + wave * 32 * AT_SP;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int r = acc_row(q, h);                         // key row inside the block = bit index
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], sl, kbk16[q]) - lq[j]);
      const bool keepb = (kwq[j] >> r) & 1u;
      *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(keepb ? pr * inv_keep : 0.f);
      const float dp = keepb ? acc2[j][q] * inv_keep : 0.f;
      acc2[j][q] = pr * (dp - dq_[j]) * p.scale;          // dS^T, kept for the second product
    }
  }
  zero16(out[0]); zero16(out[1]);
  gemm_tokens(out, slab, Gt, tp, kt, l31, h);             // dV = Pd^T dO
  {
    f32x16 dvv[2] = {out[0], out[1]};
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = acc_row(q, h);
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(acc2[j][q]);
    }
    zero16(out[0]); zero16(out[1]);
    gemm_tokens(out, slab, Qt, tp, kt, l31, h);           // dK = dS^T Q
    store_rows(out, slab, tp, p.dk + base, p.ld, row0, L, lane, l31, h);
    store_rows(dvv, slab, tp, p.dv + base, p.ld, row0, L, lane, l31, h);
  }
}

size_t attn_lds_fwd(int L) { return (size_t)2 * 128 * AT_RP + (size_t)64 * attn_tp(L) + 512; }   // slabs alias Q / K: 128 AT_SP <= 256 AT_RP
size_t attn_lds_bwd_q(int L) { return (size_t)2 * 128 * AT_RP + (size_t)64 * attn_tp(L) + 3 * 512 + 2048; }
size_t attn_lds_bwd_kv(int L) { return (size_t)2 * 128 * AT_RP + (size_t)2 * 64 * attn_tp(L) + 4 * 512 + 2048; }
size_t attn_lds_bwd(int L) { return attn_lds_bwd_kv(L) > attn_lds_bwd_q(L) ? attn_lds_bwd_kv(L) : attn_lds_bwd_q(L); }

}  // namespace

extern "C" int glr_attn_max_tokens(int backward) {
  for (int L = 128; L > 0; L -= 16)
    if ((backward ? attn_lds_bwd(L) : attn_lds_fwd(L)) <= 160 * 1024) return L;
  return 0;
}

// launches shared by the padded and the packed-rows entry points (p.L sizes the LDS: L, or the longest sentence)
static int attn_launch_fwd(const AttnParams& p, void* stream) {
  const int lds = (int)attn_lds_fwd(p.L);
  static GlrLdsAttr lds_fwd;
  if (glr_ensure_lds(lds_fwd, (const void*)k_attn_fwd, lds) != GLR_OK) return GLR_ELAUNCH;
  hipLaunchKernelGGL(k_attn_fwd, dim3(p.B * p.nh), dim3(AT_NT), lds, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}
static int attn_launch_bwd(const AttnParams& p, void* stream) {
  const int lds_q = (int)attn_lds_bwd_q(p.L), lds_kv = (int)attn_lds_bwd_kv(p.L);
  static GlrLdsAttr lds_bq, lds_bkv;
  if (glr_ensure_lds(lds_bq, (const void*)k_attn_bwd_q, lds_q) != GLR_OK) return GLR_ELAUNCH;
  if (glr_ensure_lds(lds_bkv, (const void*)k_attn_bwd_kv, lds_kv) != GLR_OK) return GLR_ELAUNCH;
  hipLaunchKernelGGL(k_attn_bwd_q, dim3(p.B * p.nh), dim3(AT_NT), lds_q, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_attn_bwd_kv, dim3(p.B * p.nh), dim3(AT_NT), lds_kv, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}
// longest sentence of a host row_start [B + 1], or 0 unless every sentence has 1 .. max_n rows
static int attn_rows_longest(const int32_t* rs, int B, int max_n) {
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    const long long n = (long long)rs[b + 1] - rs[b];
    if (rs[b] < 0 || n < 1 || n > max_n) return 0;
    if ((int)n > longest) longest = (int)n;
  }
  return longest;
}

extern "C" int glr_attn_fwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, int B, int n_heads, int L, int ld,
                            int ld_o, float scale, float p_drop, unsigned long long seed, unsigned long long offset,
                            const unsigned long long* rng_cell, void* o, float* lse, uint32_t* keep, void* stream) {
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, key_mask, B, n_heads, L, ld, ld_o, scale, p_drop, seed, offset, 128);
  if (rc != GLR_OK) return rc;
  if (!o || !lse || (p_drop > 0.f && !keep) || L > glr_attn_max_tokens(0)) return GLR_EINVAL;
  p.o = (unsigned short*)o; p.lse = lse; p.keep = keep; p.rng = rng_cell;
  return attn_launch_fwd(p, stream);
}

extern "C" int glr_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const uint8_t* key_mask,
                            const float* lse, const uint32_t* keep, int B, int n_heads, int L, int ld, int ld_o, float scale, float p_drop,
                            void* dq, void* dk, void* dv, void* stream) {
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, key_mask, B, n_heads, L, ld, ld_o, scale, p_drop, 0, 0, 128);
  if (rc != GLR_OK) return rc;
  if (!o || !d_o || !lse || !dq || !dk || !dv || (p_drop > 0.f && !keep) || L > glr_attn_max_tokens(1)) return GLR_EINVAL;
  p.o = (unsigned short*)const_cast<void*>(o); p.d_o = (const unsigned short*)d_o; p.lse = const_cast<float*>(lse);
  p.keep = const_cast<unsigned*>(keep); p.dq = (unsigned short*)dq; p.dk = (unsigned short*)dk; p.dv = (unsigned short*)dv;
  return attn_launch_bwd(p, stream);
}

extern "C" int glr_attn_rows_fwd(const void* q, const void* k, const void* v, const int32_t* row_start, const int32_t* row_start_host,
                                 int B, int n_heads, int ld, int ld_o, float scale, float p_drop, unsigned long long seed,
                                 unsigned long long offset, const unsigned long long* rng_cell, void* o, float* lse, uint32_t* keep,
                                 void* stream) {
  if (!row_start || !row_start_host || B <= 0) return GLR_EINVAL;
  const int longest = attn_rows_longest(row_start_host, B, glr_attn_max_tokens(0));
  if (longest == 0) return GLR_EINVAL;
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, nullptr, B, n_heads, longest, ld, ld_o, scale, p_drop, seed, offset, 128);
  if (rc != GLR_OK) return rc;
  if (!o || !lse || (p_drop > 0.f && !keep)) return GLR_EINVAL;
  p.o = (unsigned short*)o; p.lse = lse; p.keep = keep; p.rng = rng_cell; p.row_start = row_start;
  return attn_launch_fwd(p, stream);
}

extern "C" int glr_attn_rows_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const int32_t* row_start,
                                 const int32_t* row_start_host, const float* lse, const uint32_t* keep, int B, int n_heads, int ld,
                                 int ld_o, float scale, float p_drop, void* dq, void* dk, void* dv, void* stream) {
  if (!row_start || !row_start_host || B <= 0) return GLR_EINVAL;
  const int longest = attn_rows_longest(row_start_host, B, glr_attn_max_tokens(1));
  if (longest == 0) return GLR_EINVAL;
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, nullptr, B, n_heads, longest, ld, ld_o, scale, p_drop, 0, 0, 128);
  if (rc != GLR_OK) return rc;
  if (!o || !d_o || !lse || !dq || !dk || !dv || (p_drop > 0.f && !keep)) return GLR_EINVAL;
  p.o = (unsigned short*)const_cast<void*>(o); p.d_o = (const unsigned short*)d_o; p.lse = const_cast<float*>(lse);
  p.keep = const_cast<unsigned*>(keep); p.dq = (unsigned short*)dq; p.dk = (unsigned short*)dk; p.dv = (unsigned short*)dv;
  p.row_start = row_start;
  return attn_launch_bwd(p, stream);
}
