// Self-attention of the BERT text encoder for captions of up to 512 tokens (head size 64), forward and backward:
// softmax(Q K^T / sqrt(d) + key mask) -> dropout -> . V with the operands of glr_attn.hip, whose "a head is one score
// tile in LDS" layout ends at 128 tokens (at 512 tokens K rows + V transposed + a Q block are 155 KB of the 160 KB).
// Here one workgroup owns one 128-row block of a (sentence, head) and STREAMS the other side through LDS in 128-token
// blocks; a wave owns 32 rows, as there.  Lp = L rounded up to 128, nb = Lp / 128 blocks:
//   forward   wave = 32 query rows (fragments from global memory).  Two sweeps over the key blocks, S = Q K^T
//             recomputed (a 64-deep contraction): sweep 1 keeps a running row maximum and sum (-> lse), sweep 2 forms
//             P = exp2(s - max) / sum, normalised and dropout-scaled BEFORE its bf16 store - the rounding points of the
//             short kernel - and accumulates O += P V in registers.
//   backward  pass Q (wave = 32 queries, loop over key blocks):   S, dP = dO V^T, dS -> slab, dQ += dS K;
//             pass K (wave = 32 keys, loop over query blocks):    S^T, dP^T, P^T -> slab, dV += P^T dO, dS^T -> slab,
//             dK += dS^T Q.  Both recompute P from the saved lse; delta = <dO, O> is recomputed per block.
// No atomics, no sums across workgroups: every output row is written once by one wave, in a fixed order of blocks.
// A key block whose keys are all masked contributes exp2(-inf - finite) = 0 whether it comes first, in the middle or
// last: the running maximum only enters a subtraction once it is finite (a row with no key at all subtracts 0).
// Masked keys are not computed: per key block only the leading 32-key sub-blocks up to the last live key run (BERT's
// padding is a suffix), a block with no live key is skipped, and in pass K a wave whose keys are all masked writes zeros.
// Dropout bits: the keyed counter hash of glr_attn.hip, 16 bits per score; the counter is a function of (head index,
// query row, key) alone (include/glr.h), so it does not depend on B, L or the launch geometry.
#include "glr_attn_common.h"

namespace {

constexpr int AL_MAX = 512;           // tokens
constexpr int AL_TP = 272;            // bytes per row of a transposed [64][128 tokens] LDS block: 256 + 16

__device__ __forceinline__ float key_bias(const AttnParams& p, int b, int key) {
  return (key < p.L && (p.key_mask == nullptr || p.key_mask[(size_t)b * p.L + key] != 0)) ? 0.f : -INFINITY;
}
// kb[i] = bias of key i for i < Lp, and per 64 keys the last live one (-1: none) - what a block can skip comes from here
__device__ __forceinline__ void key_bias_fill(const AttnParams& p, int b, int Lp, float* kb, int* last64, int tid) {
  for (int i0 = 0; i0 < Lp; i0 += AT_NT) {
    const int i = i0 + tid;                      // Lp is a multiple of 128: a wave's 64 keys are all inside or all outside
    const float v = i < Lp ? key_bias(p, b, i) : -INFINITY;
    const unsigned long long live = __ballot(v == 0.f);
    if (i < Lp) {
      kb[i] = v;
      if ((tid & 63) == 0) last64[i >> 6] = live ? 63 - __builtin_clzll(live) : -1;
    }
  }
}
// leading 32-key sub-blocks of key block c that hold a live key: what lies behind them adds exp2(-inf) = 0 to every sum
// and is not computed (BERT's padding is a suffix); 0 = the whole block is skipped.  Uniform over the workgroup.
__device__ __forceinline__ int live_subblocks(const int* last64, int c) {
  const int lo = last64[2 * c], hi = last64[2 * c + 1];
  return hi >= 0 ? (64 + hi) / 32 + 1 : lo >= 0 ? lo / 32 + 1 : 0;
}
// keeps a wave-uniform `if (j < ne)` a branch: its body is not computed for the sub-blocks that are left out
__device__ __forceinline__ void uniform_branch() { asm volatile(""); }

// keep words (query row r of block qb, keys of block kc) -> LDS [128][4]; rows >= L and p_drop == 0 read as "keep"
__device__ __forceinline__ void keep_load(const AttnParams& p, int bh, int Lp, int qb, int kc, unsigned (&w)[2], int tid) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = tid + AT_NT * t, row = qb * 128 + (i >> 2);
    w[t] = (p.p_drop > 0.f && row < p.L) ? p.keep[((size_t)bh * Lp + row) * (Lp >> 5) + kc * 4 + (i & 3)] : 0xffffffffu;
  }
}

__global__ void __launch_bounds__(AT_NT, 2) k_attn_long_fwd(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int L = p.L, Lp = (L + 127) & ~127, nb = Lp >> 7;
  const int bh = blockIdx.x / nb, qb = blockIdx.x % nb, b = bh / p.nh, hd = bh % p.nh;
  unsigned char* Ks = smem;
  unsigned char* Vt = Ks + 128 * AT_RP;
  unsigned char* Ps = Vt + 64 * AL_TP;
  float* kb = reinterpret_cast<float*>(Ps + 128 * AT_SP);         // [AL_MAX]
  int* last64 = reinterpret_cast<int*>(kb + AL_MAX);              // [8]
  const size_t base = (size_t)b * L * p.ld + (size_t)hd * 64;
  const int row0 = qb * 128 + 32 * wave;
  const bool active = row0 < L;                  // a wave without query rows only takes part in the loads
  bf16x8 fq[4];
  frag_rows_load(p.q + base, p.ld, row0 + l31, L, h, fq);
  key_bias_fill(p, b, Lp, kb, last64, tid);
  __syncthreads();
  const float sl = p.scale * AT_LOG2E;
  float m[16], s[16];                            // running maximum (log2 units) and sum of the row of register q
#pragma unroll
  for (int q = 0; q < 16; ++q) { m[q] = -INFINITY; s[q] = 0.f; }
  // sweep 1: row maximum and sum
  for (int c = 0; c < nb; ++c) {
    const int ne = live_subblocks(last64, c);
    if (ne == 0) continue;
    uint4 rk[4];
    tile_load(p.k + base + (size_t)c * 128 * p.ld, p.ld, min(L - c * 128, 32 * ne), rk, tid);
    __syncthreads();                             // the previous block has been read
    tile_store_rows(rk, Ks, tid);
    __syncthreads();
    if (active) {
      f32x16 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) zero16(acc[j]);
      gemm_frag64(acc, fq, Ks, ne, l31, h);
      float kbv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) kbv[j] = kb[c * 128 + 32 * j + l31];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float v[4], mb = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < ne) { uniform_branch(); v[j] = __builtin_fmaf(acc[j][q], sl, kbv[j]); mb = fmaxf(mb, v[j]); }
        const float mn = fmaxf(m[q], half_max(mb));
        const float ms = mn == -INFINITY ? 0.f : mn;               // no live key so far: nothing to subtract
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < ne) { uniform_branch(); e += __builtin_amdgcn_exp2f(v[j] - ms); }
        s[q] = __builtin_fmaf(s[q], __builtin_amdgcn_exp2f(m[q] - ms), half_sum(e));     // m = -inf: s = 0 stays 0
        m[q] = mn;
      }
    }
  }
  const bool drop = p.p_drop > 0.f;
  const unsigned thr16 = drop ? (unsigned)(p.p_drop * 65536.f + 0.5f) : 0u;
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  if (active) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float ms = m[q] == -INFINITY ? 0.f : m[q];             // a sentence with every key masked: all-zero row
      if (l31 == 0)
        p.lse[(size_t)bh * Lp + row0 + acc_row(q, h)] = (ms + __builtin_amdgcn_logf(fmaxf(s[q], 1e-37f))) * (1.f / AT_LOG2E);
      m[q] = ms;
      s[q] = s[q] > 0.f ? 1.f / s[q] : 0.f;
    }
  }
  unsigned hk0, hk1;
  hash_key(p, hk0, hk1);
  unsigned char* slab = Ps + wave * 32 * AT_SP;
  f32x16 out[2];
  zero16(out[0]); zero16(out[1]);
  // sweep 2: P -> the wave's slab, O += P V
  for (int c = 0; c < nb; ++c) {
    const int ne = live_subblocks(last64, c);
    if (ne == 0) continue;
    const int rem = min(L - c * 128, 32 * ne), lk = (rem + 15) & ~15;
    uint4 rk[4], rv[4];
    tile_load(p.k + base + (size_t)c * 128 * p.ld, p.ld, rem, rk, tid);
    tile_load(p.v + base + (size_t)c * 128 * p.ld, p.ld, rem, rv, tid);
    __syncthreads();
    tile_store_rows(rk, Ks, tid);
    tile_store_transposed(rv, lk, Vt, AL_TP, tid);
    __syncthreads();
    if (active) {
      f32x16 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) zero16(acc[j]);
      gemm_frag64(acc, fq, Ks, ne, l31, h);
      float kbv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) kbv[j] = kb[c * 128 + 32 * j + l31];
      unsigned mw0 = 0u, mw1 = 0u;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = acc_row(q, h);
        unsigned r01 = 0u, r23 = 0u;
        if (drop) {
          const unsigned ctr = ((((unsigned)bh * (unsigned)AL_MAX + (unsigned)(row0 + r)) * 4u + (unsigned)c) * 32u + (unsigned)l31) * 2u;
          r01 = hash32(ctr, hk0, hk1);
          r23 = hash32(ctr + 1u, hk0, hk1);
        }
        const unsigned r16[4] = {r01 & 0xffffu, r01 >> 16, r23 & 0xffffu, r23 >> 16};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= ne) continue;                 // (uniform: the slab columns behind lk are not read)
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], sl, kbv[j]) - m[q]);
          const bool keepb = !drop || r16[j] >= thr16;
          if (drop) {
            const unsigned long long word = __ballot(keepb);
            if (lane == q * 4 + j) { mw0 = (unsigned)word; mw1 = (unsigned)(word >> 32); }
          }
          const float pd = keepb ? e * s[q] * inv_keep : 0.f;
          *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(pd);
        }
      }
      if (drop && (lane & 3) < ne) {             // (the words of keys that are left out stay unwritten and unread)
        const int q = lane >> 2, j = lane & 3;
        const size_t w0 = ((size_t)bh * Lp + row0 + acc_row(q, 0)) * (Lp >> 5) + c * 4 + j;
        p.keep[w0] = mw0;
        p.keep[w0 + 4 * (Lp >> 5)] = mw1;        // row + 4: the other lane half
      }
      gemm_tokens(out, slab, Vt, AL_TP, lk >> 4, l31, h);
    }
  }
  if (active) store_rows(out, slab, AL_TP, p.o + (size_t)b * L * p.ld_o + (size_t)hd * 64, p.ld_o, row0, L, lane, l31, h);
}

// pass Q: workgroup = (sentence, head, 128 queries), wave = 32 query rows, loop over key blocks.  As in the short kernel
// the slabs take the place of the K / V rows once every wave has its two score tiles (59 KB: two workgroups per CU).
__global__ void __launch_bounds__(AT_NT, 2) k_attn_long_bwd_q(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int L = p.L, Lp = (L + 127) & ~127, nb = Lp >> 7;
  const int bh = blockIdx.x / nb, qb = blockIdx.x % nb, b = bh / p.nh, hd = bh % p.nh;
  unsigned char* Ks = smem;
  unsigned char* Vs = Ks + 128 * AT_RP;
  unsigned char* Kt = Vs + 128 * AT_RP;
  unsigned char* Ps = smem;                      // slabs take the place of K / V: 128 AT_SP <= 256 AT_RP
  float* kb = reinterpret_cast<float*>(Kt + 64 * AL_TP);          // [AL_MAX]
  float* lse = kb + AL_MAX;                                       // [128] rows of this query block, log2 units
  float* delta = lse + 128;                                       // [128], rows of wave w written by wave w
  unsigned* keep = reinterpret_cast<unsigned*>(delta + 128);      // [128][4]
  int* last64 = reinterpret_cast<int*>(keep + 512);               // [8]
  const size_t base = (size_t)b * L * p.ld + (size_t)hd * 64, base_o = (size_t)b * L * p.ld_o + (size_t)hd * 64;
  const int row0 = qb * 128 + 32 * wave;
  const bool active = row0 < L;
  bf16x8 fq[4];
  {
    bf16x8 fg[4], fo[4];
    frag_rows_load(p.q + base, p.ld, row0 + l31, L, h, fq);
    frag_rows_load(p.d_o + base_o, p.ld_o, row0 + l31, L, h, fg);
    frag_rows_load(p.o + base_o, p.ld_o, row0 + l31, L, h, fo);
    key_bias_fill(p, b, Lp, kb, last64, tid);
    if (tid < 128) lse[tid] = qb * 128 + tid < L ? p.lse[(size_t)bh * Lp + qb * 128 + tid] * AT_LOG2E : 0.f;
    // delta[row] = <dO[row], O[row]>: a lane holds half of its row (the k pieces of its lane half)
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) d += dot8(__builtin_bit_cast(uint4, fg[ks]), __builtin_bit_cast(uint4, fo[ks]));
    d += __shfl_xor(d, 32, 64);
    if (h == 0) delta[32 * wave + l31] = d;
  }
  __syncthreads();
  const bool drop = p.p_drop > 0.f;
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  const float sl = p.scale * AT_LOG2E;
  unsigned char* slab = Ps + wave * 32 * AT_SP;
  f32x16 out[2];
  zero16(out[0]); zero16(out[1]);
  for (int c = 0; c < nb; ++c) {
    const int ne = live_subblocks(last64, c);
    if (ne == 0) continue;
    const int rem = min(L - c * 128, 32 * ne), lk = (rem + 15) & ~15;
    bf16x8 fg[4];                                // reloaded per block (L2): 16 registers less across the dS phase
    frag_rows_load(p.d_o + base_o, p.ld_o, row0 + l31, L, h, fg);
    {
      uint4 rk[4], rv[4];
      unsigned kw[2];
      tile_load(p.k + base + (size_t)c * 128 * p.ld, p.ld, rem, rk, tid);
      tile_load(p.v + base + (size_t)c * 128 * p.ld, p.ld, rem, rv, tid);
      keep_load(p, bh, Lp, qb, c, kw, tid);
      __syncthreads();                           // the slabs and K^T of the previous block have been read
      tile_store_rows(rk, Ks, tid);
      tile_store_rows(rv, Vs, tid);
      tile_store_transposed(rk, lk, Kt, AL_TP, tid);
      keep[tid] = kw[0]; keep[tid + AT_NT] = kw[1];
    }
    __syncthreads();
    f32x16 acc[4], acc2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { zero16(acc[j]); zero16(acc2[j]); }
    if (active) {
      gemm_frag64(acc, fq, Ks, ne, l31, h);                // S
      gemm_frag64(acc2, fg, Vs, ne, l31, h);               // dP (before the dropout scaling) = dO V^T
    }
    __syncthreads();                             // K / V rows are dead: their space becomes the slabs
    if (active) {
      float kbv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) kbv[j] = kb[c * 128 + 32 * j + l31];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = acc_row(q, h);
        const float lr = lse[32 * wave + r], dl = delta[32 * wave + r];
        const uint4 kw = *reinterpret_cast<const uint4*>(keep + (32 * wave + r) * 4);
        const unsigned kwj[4] = {kw.x, kw.y, kw.z, kw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= ne) continue;
          const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], sl, kbv[j]) - lr);
          const float dp = ((kwj[j] >> l31) & 1u) ? acc2[j][q] * inv_keep : 0.f;
          *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(pr * (dp - dl) * p.scale);
        }
      }
      gemm_tokens(out, slab, Kt, AL_TP, lk >> 4, l31, h);  // dQ += dS K
    }
  }
  if (active) store_rows(out, slab, AL_TP, p.dq + base, p.ld, row0, L, lane, l31, h);
}

// pass K: workgroup = (sentence, head, 128 keys), wave = 32 key rows, loop over query blocks, dK / dV in registers
__global__ void __launch_bounds__(AT_NT, 2) k_attn_long_bwd_kv(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int L = p.L, Lp = (L + 127) & ~127, nb = Lp >> 7;
  const int bh = blockIdx.x / nb, kc = blockIdx.x % nb, b = bh / p.nh, hd = bh % p.nh;
  unsigned char* Qs = smem;
  unsigned char* Gs = Qs + 128 * AT_RP;          // dO
  unsigned char* Qt = Gs + 128 * AT_RP;
  unsigned char* Gt = Qt + 64 * AL_TP;
  unsigned char* Ps = smem;                      // slabs take the place of Q / dO rows
  float* lse = reinterpret_cast<float*>(Gt + 64 * AL_TP);         // [128] rows of the current query block, log2 units
  float* delta = lse + 128;                                       // [2][128] partial sums (the two thread halves)
  unsigned* keep = reinterpret_cast<unsigned*>(delta + 256);      // [128][4]
  float* kb = reinterpret_cast<float*>(keep + 512);               // [128] keys of this block
  const size_t base = (size_t)b * L * p.ld + (size_t)hd * 64, base_o = (size_t)b * L * p.ld_o + (size_t)hd * 64;
  const int row0 = kc * 128 + 32 * wave;
  const bool active = row0 < L;
  const float kbt = tid < 128 ? key_bias(p, b, kc * 128 + tid) : -INFINITY;
  if (tid < 128) kb[tid] = kbt;
  const bool blk_live = __syncthreads_or(kbt == 0.f);             // no live key in the block: dK = dV = 0, nothing to read
  // a wave whose 32 keys are all masked (BERT's padding) only takes part in the loads: its dK / dV rows are zero
  const bool compute = active && __ballot(kb[32 * wave + l31] == 0.f) != 0ull;
  const bool drop = p.p_drop > 0.f;
  const float inv_keep = drop ? 1.f / (1.f - p.p_drop) : 1.f;
  const float sl = p.scale * AT_LOG2E;
  unsigned char* slab = Ps + wave * 32 * AT_SP;
  f32x16 dk[2], dv[2];
  zero16(dk[0]); zero16(dk[1]); zero16(dv[0]); zero16(dv[1]);
  for (int c = 0; c < (blk_live ? nb : 0); ++c) {
    const int rem = L - c * 128, lk = min(128, (rem + 15) & ~15), nqb = min(4, (rem + 31) >> 5);
    bf16x8 fk[4], fv[4];                         // reloaded per block (L2): the accumulators need the registers
    frag_rows_load(p.k + base, p.ld, row0 + l31, L, h, fk);
    frag_rows_load(p.v + base, p.ld, row0 + l31, L, h, fv);
    {
      uint4 rq[4], rg[4], ro[4];
      unsigned kw[2];
      const size_t blk = (size_t)c * 128;
      tile_load(p.q + base + blk * p.ld, p.ld, rem, rq, tid);
      tile_load(p.d_o + base_o + blk * p.ld_o, p.ld_o, rem, rg, tid);
      tile_load(p.o + base_o + blk * p.ld_o, p.ld_o, rem, ro, tid);
      keep_load(p, bh, Lp, c, kc, kw, tid);
      const float lr = (tid < 128 && tid < rem) ? p.lse[(size_t)bh * Lp + c * 128 + tid] * AT_LOG2E : 0.f;
      __syncthreads();                           // the slabs, Q^T and dO^T of the previous block have been read
      tile_store_rows(rq, Qs, tid);
      tile_store_rows(rg, Gs, tid);
      tile_store_transposed(rq, lk, Qt, AL_TP, tid);
      tile_store_transposed(rg, lk, Gt, AL_TP, tid);
      keep[tid] = kw[0]; keep[tid + AT_NT] = kw[1];
      if (tid < 128) lse[tid] = lr;
      delta[tid] = (dot8(rg[0], ro[0]) + dot8(rg[1], ro[1])) + (dot8(rg[2], ro[2]) + dot8(rg[3], ro[3]));
    }
    __syncthreads();
    f32x16 acc[4], acc2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { zero16(acc[j]); zero16(acc2[j]); }
    float lq[4], dq_[4];
    unsigned kwq[4];
    if (compute) {
      gemm_frag64(acc, fk, Qs, nqb, l31, h);               // S^T
      gemm_frag64(acc2, fv, Gs, nqb, l31, h);              // dP^T = V dO^T
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lq[j] = lse[32 * j + l31];
      dq_[j] = delta[32 * j + l31] + delta[128 + 32 * j + l31];
      kwq[j] = keep[(32 * j + l31) * 4 + wave];            // keys of this wave's 32, of query 32 j + l31
    }
    __syncthreads();                             // Q / dO rows are dead: their space becomes the slabs
    if (compute) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = acc_row(q, h);                       // key row inside the wave's 32 = bit index
        const float kbk = kb[32 * wave + r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= nqb) continue;                          // (uniform: queries >= L; the slab columns behind lk are not read)
          const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], sl, kbk) - lq[j]);
          const bool keepb = (kwq[j] >> r) & 1u;
          *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(keepb ? pr * inv_keep : 0.f);
          const float dp = keepb ? acc2[j][q] * inv_keep : 0.f;
          acc2[j][q] = pr * (dp - dq_[j]) * p.scale;        // dS^T, kept for the second product
        }
      }
      gemm_tokens(dv, slab, Gt, AL_TP, lk >> 4, l31, h);   // dV += Pd^T dO
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = acc_row(q, h);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nqb) *reinterpret_cast<unsigned short*>(slab + r * AT_SP + (32 * j + l31) * 2) = f2bf(acc2[j][q]);
      }
      gemm_tokens(dk, slab, Qt, AL_TP, lk >> 4, l31, h);   // dK += dS^T Q
    }
  }
  if (active) {
    store_rows(dk, slab, AL_TP, p.dk + base, p.ld, row0, L, lane, l31, h);
    store_rows(dv, slab, AL_TP, p.dv + base, p.ld, row0, L, lane, l31, h);
  }
}

constexpr int AL_LDS_FWD = 128 * AT_RP + 64 * AL_TP + 128 * AT_SP + AL_MAX * 4 + 64;
constexpr int AL_LDS_BWD_Q = 2 * 128 * AT_RP + 64 * AL_TP + AL_MAX * 4 + 2 * 512 + 2048 + 64;
constexpr int AL_LDS_BWD_KV = 2 * 128 * AT_RP + 2 * 64 * AL_TP + 4 * 512 + 2048;
static_assert(128 * AT_SP <= 2 * 128 * AT_RP, "the slabs take the place of two row-major operands");
static_assert(AL_LDS_FWD <= 80 * 1024 && AL_LDS_BWD_Q <= 80 * 1024 && AL_LDS_BWD_KV <= 80 * 1024, "two workgroups per CU");

}  // namespace

extern "C" int glr_attn_long_max_tokens(void) { return AL_MAX; }

extern "C" int glr_attn_long_fwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, int B, int n_heads, int L,
                                 int ld, int ld_o, float scale, float p_drop, unsigned long long seed, unsigned long long offset,
                                 const unsigned long long* rng_cell, void* o, float* lse, uint32_t* keep, void* stream) {
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, key_mask, B, n_heads, L, ld, ld_o, scale, p_drop, seed, offset, AL_MAX);
  if (rc != GLR_OK) return rc;
  if (!o || !lse || (p_drop > 0.f && !keep)) return GLR_EINVAL;
  p.o = (unsigned short*)o; p.lse = lse; p.keep = keep; p.rng = rng_cell;
  static GlrLdsAttr lds_fwd;
  if (glr_ensure_lds(lds_fwd, (const void*)k_attn_long_fwd, AL_LDS_FWD) != GLR_OK) return GLR_ELAUNCH;
  const int nb = (L + 127) >> 7;
  hipLaunchKernelGGL(k_attn_long_fwd, dim3(B * n_heads * nb), dim3(AT_NT), AL_LDS_FWD, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_attn_long_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const uint8_t* key_mask,
                                 const float* lse, const uint32_t* keep, int B, int n_heads, int L, int ld, int ld_o, float scale,
                                 float p_drop, void* dq, void* dk, void* dv, void* stream) {
  AttnParams p;
  const int rc = attn_fill(p, q, k, v, key_mask, B, n_heads, L, ld, ld_o, scale, p_drop, 0, 0, AL_MAX);
  if (rc != GLR_OK) return rc;
  if (!o || !d_o || !lse || !dq || !dk || !dv || (p_drop > 0.f && !keep)) return GLR_EINVAL;
  p.o = (unsigned short*)const_cast<void*>(o); p.d_o = (const unsigned short*)d_o; p.lse = const_cast<float*>(lse);
  p.keep = const_cast<unsigned*>(keep); p.dq = (unsigned short*)dq; p.dk = (unsigned short*)dk; p.dv = (unsigned short*)dv;
  static GlrLdsAttr lds_bq, lds_bkv;
  if (glr_ensure_lds(lds_bq, (const void*)k_attn_long_bwd_q, AL_LDS_BWD_Q) != GLR_OK) return GLR_ELAUNCH;
  if (glr_ensure_lds(lds_bkv, (const void*)k_attn_long_bwd_kv, AL_LDS_BWD_KV) != GLR_OK) return GLR_ELAUNCH;
  const int nb = (L + 127) >> 7;
  hipLaunchKernelGGL(k_attn_long_bwd_q, dim3(B * n_heads * nb), dim3(AT_NT), AL_LDS_BWD_Q, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_attn_long_bwd_kv, dim3(B * n_heads * nb), dim3(AT_NT), AL_LDS_BWD_KV, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}
