// K1: fused region x word attention + cosine similarity + log-sum-exp, forward AND backward.
//
// Replaces, for every (image b, sentence i) pair at once, the body of the reference sentence loop:
// attention_fn (/root/reference/gloria/loss/gloria_loss.py:19-63), cosine_similarity (:11-16) and the
// exp/sum/log of local_loss (:150-158, :164) - and, in the backward variant, autograd through them.
//
// Maths, per image b and word w of sentence i, regions r:
//   s[w,r]  = <T_w, V_r>                          a1 = softmax over the words of the sentence
//   e2[w,r] = exp(temp1 * a1[w,r])                Z_w = sum_r e2,   a2 = e2 / Z_w
//   c_w     = sum_r a2[w,r] V_r                   dot_w = <T_w, c_w> = sum_r a2[w,r] s[w,r]
//   |c_w|^2 = sum_r a2[w,r] u[w,r],  u[w,r] = <V_r, c_w> = sum_r' a2[w,r'] G[r,r'],  G = V^T V (Gram)
// so the weighted context itself is never formed: the second contraction runs against the
// S x S Gram matrix of the image (K = S instead of K = D) and both cosine ingredients are
// region-sums of products that already sit in the MFMA accumulators.
//
// One workgroup (8 waves, 512 threads) = one image b x one tile of 64 word slots (whole sentences).
//   P1  acc[w,r] = T_tile . V_b^T            MFMA 32x32, K = D.  T tile (64 rows) and vt[b] (S_pad
//       rows, [region][feature]) stream HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4) into a
//       2-deep ring; the LDS image is lane-linear, bank conflicts are removed by an XOR swizzle of
//       the 16-byte slot applied on the SOURCE address and again on the fragment read.
//   P2  forward: scores -> LDS fp32 tile; one thread per region column walks the words of each
//       sentence for log-sum-exp statistics lse[r, sentence] (kept for backward).
//       Then, from the scores still in registers: a1 = exp(s - lse), e2 = exp(temp1 a1) -> LDS image
//       [word][region] in the operand dtype; per-word Z and dot~ by butterfly reductions.
//       (backward: lse comes from the forward, no walk.)
//   P3  acc[w,r] (+)= E . G_b^T              MFMA 32x32, K = S_pad, A operand = the LDS image,
//       gram[b] rows streamed through the same ring.
//   P4  forward: |c|^2 from acc, cosine, per-sentence aggregate -> sim[b, i]; optional diagonal
//       attention maps.
//       backward: with per-word scalars alpha, beta, kappa derived from dsim and the saved stats the
//       accumulator is initialised with -alpha*s and the image holds beta*a2, so P3 leaves -da2;
//       softmax backward over regions (needs kappa only) and over words (segment sums by LDS
//       atomics) gives ds; outputs X = ds + alpha*a2 and a2 (+ per-word beta, gamma) for the gradient GEMMs.
//
// Sentences longer than one tile own ceil(n/64) consecutive tiles, processed by the workgroup of
// their first tile in two sweeps (statistics, then results).
//
// Wave w: wm = w & 1 -> 32-word block; wg = w >> 1 -> region blocks {wg, wg+4, wg+8}.
// Accumulator element q of a block: word row (q&3) + 8*(q>>2) + 4*(lane>>5), region column lane&31.
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "glr_k1.h"

#ifndef GLR_STAGGER
#define GLR_STAGGER 1
#endif

extern "C" int glr_region_pad(int s_eff) { return (s_eff + 63) / 64 * 64; }
// populated word slots per 64-slot tile: the fp32 mode keeps a 32-word score tile + fp32 image in LDS
extern "C" int glr_tile_capacity(int op_dtype) { return op_dtype == GLR_F32 ? 32 : GLR_TILE_WORDS; }

namespace {

constexpr int NTHR = 512;

#ifdef GLR_STAMPS
// per-wave stamps inside the P1 stream of the pair kernel: [workgroup][wave][chunk][3] = after the barrier,
// after the DMA issue, after the MFMAs (tools/stamps_k1.py waves)
__device__ unsigned long long* g_wave_stamps = nullptr;
#define GLR_WSTAMP(c, k)                                                                               \
  do {                                                                                                 \
    if (NH == 2 && !A_RES && g_wave_stamps != nullptr && (lane == 0) && blockIdx.x < 4096) {            \
      unsigned long long t_;                                                                           \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                       \
      g_wave_stamps[(((size_t)blockIdx.x * 8 + wave) * 32 + (c)) * 3 + (k)] = t_;                       \
    }                                                                                                  \
  } while (0)
#define GLR_STAMP(i)                                                                        \
  do {                                                                                      \
    if (tid == 0 && p.stamps) {                                                             \
      unsigned long long t_;                                                                \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
      p.stamps[(size_t)blockIdx.x * 12 + (i)] = t_;                                          \
    }                                                                                       \
  } while (0)
#define GLR_STAMP2(i)                                                                       \
  do {                                                                                      \
    if (tid == 0 && p.stamps2) {                                                            \
      unsigned long long t_;                                                                \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
      p.stamps2[(size_t)blockIdx.x * 12 + (i)] = t_;                                         \
    }                                                                                       \
  } while (0)
#else
#define GLR_STAMP(i)
#define GLR_STAMP2(i)
#define GLR_WSTAMP(c, k)
#endif
// timing-only diagnostic build (make ablate): a phase is skipped when its bit is set in GLR_K1_DBG - results are
// garbage, only the run time matters (tools/ablate_k1.py); never compiled into libglr.so
#ifdef GLR_ABLATE
#define GLR_SKIP(bit) (p.dbg & (bit))
#else
#define GLR_SKIP(bit) false
#endif

// 16-byte streaming store of a kernel output: non-temporal, so that the backward's 300 KB of outputs per workgroup do
// not evict the operand streams (vt / gram / word tiles) the XCD's other workgroups are re-reading from L2
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_stream16(void* dst, const uint4 v, bool plain = false) {
  u32x4 x = {v.x, v.y, v.z, v.w};
  if (plain) *reinterpret_cast<u32x4*>(dst) = x;
  else __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned char*)p;
}
// one LDS-DMA piece: lane i writes 16 B at lds_dst + 16*i, read from its own gsrc (asm: hipcc's
// waitcnt pass would otherwise drain every in-flight DMA before each ds_read)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): own LDS traffic done (vmcnt untouched)
  __builtin_amdgcn_s_barrier();
}

constexpr int CHB = 64;     // bytes of K per ring row (both dtypes): bf16 = 2 k-steps of 16, fp32 = 2 of 8
constexpr int NBUF = 4;     // ring depth
[[maybe_unused]] constexpr int PD = 3;       // chunks issued ahead of the one being consumed (documentation of the ring depth)

// acc[j] (+)= A(tw words x K) . Bt(brows x K)^T for this wave's blocks.
//   A_RES = false: A rows stream from `asrc` (tw rows per 64-row tile block, apitch = K bytes per row) together with B.
//   A_RES = true : A fragments come from the LDS image `aimg` ([word][k], pitch aimg_pitch bytes).
// B rows stream from `bsrc` (one block of brows rows).  K bytes = nchunk * CHB.  Both operands are K-tiled
// (glr_tile_k: [K chunk][row][CHB bytes] per block).
// NPWC = LDS-DMA pieces every wave issues per chunk (compile time, so every vmcnt wait is an immediate).
//
// Ring protocol (NBUF buffers, PD chunks ahead, ONE barrier per chunk): at step c every wave waits
// for its own DMA pieces of chunk c (counted vmcnt leaves the PD-1 younger chunks in flight),
// the barrier then publishes chunk c AND proves every wave finished reading chunk c-1, whose
// buffer is the target of the DMA for chunk c+PD issued right after the barrier.
// Measured (tools/stamps_k1.py): the streams run at ~27 B/clk/CU of L2->LDS DMA issue, independent of the
// prefetch depth and of reading fragments one chunk ahead; fewer DMA-issuing waves are slower.
// A rows of this wave: ring / image row `arow0 + (lane & 31)` feeds acc; with NH == 2 a second 32-row block
// `a2_delta` BYTES further on feeds acc2 (another tile's rows, or the second word block of the same tile).
template <typename O, bool A_RES, int NPWC, int NH = 1, int NB = NBUF>
__device__ __forceinline__ void stream_gemm_n(f32x16 (&acc)[3], f32x16 (&acc2)[3], int arow0, int a2_delta, unsigned char* ring,
                                              int buf_bytes,
                                              const unsigned char* asrc, size_t apitch,
                                              const unsigned char* bsrc, size_t bpitch, int brows, int nchunk,
                                              const unsigned char* aimg, int aimg_pitch, int wave, int lane, int wm,
                                              int wg, int nrb, int tw) {
  constexpr int KSTEPS = CHB / 32, RPI = 16;          // a 1-KiB DMA piece = half a 32-row block (2 of its 4 slots)
  constexpr int PDD = NB - 1;                          // chunks issued ahead; buffer (c+PDD) % NB == (c-1) % NB
  constexpr bool STAG = GLR_STAGGER && PDD == 3;
  static_assert(PDD == 1 || PDD == 3, "wait immediates are written for 2- and 4-deep rings");
  // the per-lane address tables below are loop invariant w.r.t. the caller's tile loops; laundering the
  // lane id keeps hipcc from hoisting all of them (x8 template instances) to kernel entry, where they
  // would stay live through every phase and push the kernel into scratch spills
  asm volatile("" : "+v"(lane));
  const int l31 = lane & 31, h = lane >> 5;
  const int arows = A_RES ? 0 : NH * tw;               // NH tiles of tw populated rows (one tile = TW slots)
  const bool active = wm * 32 < tw;                    // fp32 tiles hold 32 words: odd waves only move data
  const int winstr = (arows + brows) / RPI;            // 1-KiB DMA pieces per chunk
  const unsigned ring_lds = lds_addr(ring);
  // The ring buffer holds a chunk exactly as HBM does (glr_k1.h, glr_ktile_off): [32-row block][16-byte slot][row].
  // A DMA piece is then a LINEAR 1-KiB copy, and the fragment a lane reads for k-step kk of a block - slot kk * 2 + h,
  // row l31 - sits at consecutive 16-byte addresses along the lanes of a half: conflict-free without any swizzle.
  int koff[KSTEPS];                                    // byte offset of k-step kk inside a 32-row block
#pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) koff[kk] = (kk * 2 + h) * 512 + l31 * 16;
  // Region blocks this wave does not own (small S_pad only) are clamped to a valid row block and their
  // accumulators are simply never read: NO branches inside the k loop (a guarded load+MFMA pair compiles
  // to load / wait / MFMA in its own basic block and serialises on the LDS latency)
  int bofs[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) bofs[j] = (arows / 32 + min(wg + 4 * j, nrb - 1)) * 2048;

  // every wave issues exactly NPWC pieces per chunk (piece indices past the end are clamped to the
  // last piece: two waves then write the same bytes to the same LDS slot, which is harmless)
  const unsigned char* psrc[NPWC];
  unsigned pdst[NPWC];
  int pstep[NPWC];
#pragma unroll
  for (int i = 0; i < NPWC; ++i) {
    const int k = min(wave + 8 * i, winstr - 1);
    const int row0 = (k >> 1) * 32;                    // first ring row of the piece's block; its half: k & 1
    // A rows of the ring = populated rows [0, tw) of tile (row / tw); a tile block holds TW rows per chunk in HBM.
    const bool is_a = row0 < arows;
    const int tl = row0 / tw, rr0 = row0 - tl * tw;
    const size_t off = is_a ? (size_t)tl * TW * apitch + (size_t)(rr0 / 32) * 2048 : (size_t)((row0 - arows) / 32) * 2048;
    psrc[i] = (is_a ? asrc : bsrc) + off + (k & 1) * 1024 + lane * 16;
    pstep[i] = (is_a ? TW : brows) * CHB;                    // bytes from one K chunk to the next
    pdst[i] = ring_lds + k * 1024;
  }
  auto issue = [&](int c) {
    const unsigned boff = (c % NB) * buf_bytes;
#pragma unroll
    for (int i = 0; i < NPWC; ++i) glds16(psrc[i] + (size_t)((unsigned)c * (unsigned)pstep[i]), pdst[i] + boff);
  };
  auto compute = [&](int c) {
    const unsigned char* rb = ring + (c % NB) * buf_bytes;
    if (active) {
      const unsigned char* aa0 = A_RES ? (aimg + (arow0 + l31) * aimg_pitch + c * CHB + h * 16)
                                       : (rb + (arow0 / 32) * 2048);
      typename O::frag fa[KSTEPS], fa2[KSTEPS], fb[KSTEPS][3];
#pragma unroll
      for (int kk = 0; kk < KSTEPS; ++kk) {
        fa[kk] = A_RES ? O::ld(aa0 + kk * 32) : O::ld(aa0 + koff[kk]);
        if (NH == 2) fa2[kk] = A_RES ? O::ld(aa0 + a2_delta + kk * 32) : O::ld(aa0 + a2_delta + koff[kk]);
#pragma unroll
        for (int j = 0; j < 3; ++j) fb[kk][j] = O::ld(rb + bofs[j] + koff[kk]);
      }
      // keep all fragment reads in flight together: without this fence hipcc re-serialises them into
      // read / wait / MFMA triples
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < KSTEPS; ++kk)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          O::mma(fa[kk], fb[kk][j], acc[j]);
          if (NH == 2) O::mma(fa2[kk], fb[kk][j], acc2[j]);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Waves w and w + 4 share a SIMD and leave every barrier together.  If both first issue their DMA pieces
  // (~100 cycles of issue each) the matrix pipe idles meanwhile and is contended afterwards, so (4-deep ring
  // only) waves 4-7 issue AFTER their MFMAs: one partner's DMA issue overlaps the other's matrix work.
  const bool late = STAG && wave >= 4;
  for (int c = 0; c < PDD && c < nchunk; ++c) issue(c);
  int c = 0;
  for (; c + PDD <= nchunk; ++c) {                       // steady state: PDD-1 younger chunks stay in flight
    wait_vm<(PDD - 1) * NPWC>();
    wg_barrier();
    GLR_WSTAMP(c, 0);
    if (!late && c + PDD < nchunk) issue(c + PDD);
    GLR_WSTAMP(c, 1);
    compute(c);
    if (late && c + PDD < nchunk) issue(c + PDD);
    GLR_WSTAMP(c, 2);
  }
  for (; c < nchunk; ++c) {                              // tail (PDD == 3 only): nchunk-1-c younger chunks in flight
    if (nchunk - 1 - c == 1) wait_vm<NPWC>(); else wait_vm<0>();
    wg_barrier();
    compute(c);
  }
  wg_barrier();                                          // every wave is done with the ring
}

template <typename O, bool A_RES, int NH = 1, int NB = NBUF>
__device__ __forceinline__ void stream_gemm(f32x16 (&acc)[3], f32x16 (&acc2)[3], int arow0, int a2_delta, unsigned char* ring,
                                            int buf_bytes, const unsigned char* asrc, size_t apitch,
                                            const unsigned char* bsrc, size_t bpitch, int brows, int nchunk,
                                            const unsigned char* aimg, int aimg_pitch, int wave, int lane, int wm,
                                            int wg, int nrb, int tw) {
  constexpr int RPI = 64 / (CHB / 16);
  const int winstr = ((A_RES ? 0 : NH * tw) + brows) / RPI;
  const int npw = (winstr + 7) / 8;                      // workgroup-uniform
#define GLR_SG(N) stream_gemm_n<O, A_RES, N, NH, NB>(acc, acc2, arow0, a2_delta, ring, buf_bytes, asrc, apitch, bsrc, bpitch, brows, \
                                                 nchunk, aimg, aimg_pitch, wave, lane, wm, wg, nrb, tw)
  switch (npw) {
    case 1: GLR_SG(1); break;
    case 2: GLR_SG(2); break;
    case 3: GLR_SG(3); break;
    default: GLR_SG(4); break;
  }
#undef GLR_SG
}

// ---- cross-lane sums without LDS traffic: DPP row_shr adds; lane 15 of every 16-lane row ends
// up holding that row's total (the other lanes hold partial prefixes)
template <int N>
__device__ __forceinline__ float dpp_shr(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x110 + N, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp_shr<1>(v);
  v += dpp_shr<2>(v);
  v += dpp_shr<4>(v);
  v += dpp_shr<8>(v);
  return v;
}

// FULL: S_pad == GLR_MAX_SPAD (the production shape, 361/362 regions): every wave owns three valid region
// blocks, so the per-block guards vanish at compile time (a guarded LDS access compiles to its own basic
// block with a full s_waitcnt: 48 serialised LDS round trips per phase otherwise).
#define GLR_BLK_OK(blk) (FULL || (blk) < nrb)
// AUX (backward only): extra gradient inputs - `damean` (word-mean attention rows, regularisers) and `dattn`
// (diagonal attention maps, attention supervision).  A separate instance: their live values cost the plain
// backward ~90 spilled registers (3.0 -> 5.5 ms) when compiled in unconditionally.
template <typename O, bool BWD, bool FULL, bool AUX>
__global__ void __launch_bounds__(NTHR) k_local_attn(LaParams p) {
  constexpr int ESZ = O::ESZ, CB = CHB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wg = wave >> 1;
  const int l31 = lane & 31, h = lane >> 5;

  // ---- block -> (image, tile).  Blocks that share blockIdx % 8 share an XCD (speed only):
  // all tiles of one image go to one XCD so vt[b] / gram[b] stay in that XCD's L2.
  int b, tile0;
  if (p.pair_only) {
    b = blockIdx.x;
    tile0 = p.sent_slot0[p.img_offset + b] / TW;
  } else {
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    b = (q / p.n_items) * 8 + xcd;
    if (b >= p.B_img) return;
    tile0 = p.item_tile[q % p.n_items];
  }
  int nsub = p.tile_nsub[tile0];      // 0: ordinary tile, k > 1: head of a k-tile sentence, < 0: continuation
  if (nsub < 0) return;
  if (nsub == 0) nsub = 1;

  const int S_pad = FULL ? GLR_MAX_SPAD : p.S_pad, D = p.D;
  // LDS tile pitches are compile-time constants (sized for GLR_MAX_SPAD) so that every per-element
  // LDS address is one lane-dependent base + an immediate offset
  constexpr int SCP = GLR_MAX_SPAD;                  // fp32 score tile pitch (floats)
  constexpr int IMP = GLR_MAX_SPAD * ESZ + 16;       // LDS image pitch (bytes)
  const int nrb = S_pad >> 5;
  const int tw = ESZ == 2 ? TW : p.tw;               // bf16 tiles are always full width
  const bool wactive = ESZ == 2 || wm * 32 < tw;

  unsigned char* ring = smem;                // ring buffers / score tile / rho share [0, off_img)
  float* sc = reinterpret_cast<float*>(smem);
  unsigned char* img = smem + p.off_img;
  int* seg_w0 = reinterpret_cast<int*>(smem + p.off_small);
  int* seg_n = seg_w0 + TW;
  int* seg_sent = seg_n + TW;
  int* wseg = seg_sent + TW;                          // [TW] segment of each word slot (-1 = empty)
  float* red = reinterpret_cast<float*>(wseg + TW);   // [3][8][TW]  (bwd: al, be, ka, zi per word)
  float* zsum = red + 24 * TW;                        // [TW]
  float* exs = zsum + TW;                             // [TW]
  int* diag = reinterpret_cast<int*>(exs + TW);       // [0] = w0, [1] = n of the diagonal sentence
  float* aggv = reinterpret_cast<float*>(diag + 2);
  float* mrun = aggv + 2;                             // [S_pad] running max / lse (multi-tile)
  float* srun = mrun + GLR_MAX_SPAD;                  // [S_pad] running sum / rho (multi-tile bwd)
  float* w_al = red;                                  // bwd per-word scalars
  float* w_be = red + TW;
  float* w_ka = red + 2 * TW;
  float* w_zi = red + 3 * TW;

  const int seg_first = p.tile_first[tile0];
  const int long_sent = p.order[seg_first];
  const int long_n = p.cap_lens[long_sent];
  const size_t rowbytes1 = (size_t)D * ESZ;
  const size_t rowbytes2 = (size_t)S_pad * ESZ;
  const unsigned char* vt_b = p.vt + (size_t)b * S_pad * rowbytes1;
  const unsigned char* gram_b = p.gram + (size_t)b * S_pad * rowbytes2;
  const int buf1 = (tw + S_pad) * CB, buf2 = S_pad * CB;
  const int nch1 = (int)(rowbytes1 / CB), nch2 = (int)(rowbytes2 / CB);
  if (nsub > 1) {
    if (tid < S_pad) { mrun[tid] = -INFINITY; srun[tid] = 0.f; }
    if (tid == 0) aggv[0] = 0.f;
  }

  f32x16 acc[3];
  f32x16 a1r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) a1r[j][q] = 0.f;

  for (int sweep = (nsub > 1 ? 0 : 1); sweep < 2; ++sweep)
  for (int sub = 0; sub < nsub; ++sub) {
    const int tile = tile0 + sub;
    __syncthreads();          // previous iteration's LDS readers are done
    int nseg;
    if (nsub > 1) {
      nseg = 1;
      if (tid == 0) { seg_sent[0] = long_sent; seg_w0[0] = 0; seg_n[0] = min(tw, long_n - sub * tw); }
    } else {
      nseg = p.tile_first[tile + 1] - seg_first;
      if (tid < nseg) {
        const int sent = p.order[seg_first + tid];
        seg_sent[tid] = sent;
        seg_w0[tid] = p.sent_slot0[sent] - tile * TW;
        seg_n[tid] = p.cap_lens[sent];
      }
    }
    if (tid < TW) wseg[tid] = -1;
    if (tid == 0) { diag[0] = 0; diag[1] = 0; }
    __syncthreads();
    if (tid < nseg) {
      const int w0 = seg_w0[tid], n = seg_n[tid];
      for (int w = 0; w < n; ++w) wseg[w0 + w] = tid;
      if (seg_sent[tid] == p.img_offset + b) { diag[0] = w0; diag[1] = n; }
    }
    __syncthreads();
    const int wbase = (nsub > 1) ? sub * tw : 0;   // index of slot 0's word inside its sentence (multi-tile)

    if (BWD) {
      // per-word scalars from dsim and the forward's saved statistics
      if (tid < TW) {
        const int sg = wseg[tid];
        float al = 0.f, be = 0.f, ka = 0.f, zi = 0.f, ga = 0.f;
        const size_t slot = (size_t)tile * TW + tid;
        if (sg >= 0) {
          const int sent = seg_sent[sg];
          const float g = p.dsim[(size_t)b * p.ld_sim + sent];
          const float* ws = p.wstat + ((size_t)b * p.n_slots + slot) * WSTAT;
          const float Z = ws[0], cosv = ws[1], nc2 = ws[2];
          const float tn = p.tnorm[slot];
          float A = __expf(p.sim[(size_t)b * p.ld_sim + sent] / p.temp3);
          if (p.agg == GLR_AGG_MEAN) A *= (float)p.cap_lens[sent];
          const float q = g * p.temp3 * p.temp2 * __expf(p.temp2 * cosv) / A;
          const float nc = sqrtf(nc2);
          const float prod = tn * nc;
          const float den = fmaxf(prod, p.eps);
          al = q / den;
          if (prod >= p.eps) { be = q * cosv / nc2; ga = q * cosv / (tn * tn); }
          ka = al * (cosv * den) - be * nc2;
          zi = Z > 0.f ? 1.f / Z : 0.f;
        }
        w_al[tid] = al; w_be[tid] = be; w_ka[tid] = ka; w_zi[tid] = zi;
        if (sweep == 1) { p.gamma[(size_t)b * p.n_slots + slot] = ga; p.beta[(size_t)b * p.n_slots + slot] = be; }
      }
    }

    GLR_STAMP(0);
    // ================= P1: acc[w, r] = T . V^T =================
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    stream_gemm<O, false>(acc, acc, wm * 32, 0, ring, buf1, p.tp + (size_t)tile * TW * rowbytes1, rowbytes1, vt_b, rowbytes1, S_pad,
                          nch1, nullptr, 0, wave, lane, wm, wg, nrb, tw);

    GLR_STAMP(1);
    if (!BWD) {
      // scores -> LDS fp32 tile sc[word][region] (aliases the ring: every wave passed the last barrier)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int blk = wg + 4 * j;
        if (GLR_BLK_OK(blk) && wactive) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
            sc[word * SCP + blk * 32 + l31] = acc[j][q];
          }
        }
      }
      __syncthreads();
      // column walk: log-sum-exp over the words of each sentence, one thread per region.
      // The result overwrites row `s` of the thread's own column (row s <= first word of segment s).
      if (tid < S_pad) {
        const int r = tid;
        if (nsub > 1) {
          if (sweep == 0) {
            const int n = seg_n[0];
            float m = mrun[r];
            for (int w = 0; w < n; ++w) m = fmaxf(m, sc[w * SCP + r]);
            float sum = srun[r] * __expf(mrun[r] - m);
            for (int w = 0; w < n; ++w) sum += __expf(sc[w * SCP + r] - m);
            mrun[r] = m;
            srun[r] = sum;
            if (sub == nsub - 1) {                       // final statistics of the sentence
              const float l = m + __logf(sum);
              mrun[r] = l;
              if (p.lse) p.lse[((size_t)b * p.n_sent + long_sent) * S_pad + r] = l;
            }
          }
        } else {
          for (int s = 0; s < nseg; ++s) {
            const int w0 = seg_w0[s], n = seg_n[s];
            const float* col = sc + w0 * SCP + r;
            float m = -INFINITY;
            int w = 0;
            for (; w + 4 <= n; w += 4) {               // 4 independent LDS reads in flight
              const float x0 = col[w * SCP], x1 = col[(w + 1) * SCP], x2 = col[(w + 2) * SCP], x3 = col[(w + 3) * SCP];
              m = fmaxf(m, fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)));
            }
            for (; w < n; ++w) m = fmaxf(m, col[w * SCP]);
            float sum = 0.f;
            for (w = 0; w + 4 <= n; w += 4) {
              const float x0 = col[w * SCP], x1 = col[(w + 1) * SCP], x2 = col[(w + 2) * SCP], x3 = col[(w + 3) * SCP];
              sum += (__expf(x0 - m) + __expf(x1 - m)) + (__expf(x2 - m) + __expf(x3 - m));
            }
            for (; w < n; ++w) sum += __expf(col[w * SCP] - m);
            const float l = m + __logf(sum);
            sc[s * SCP + r] = l;
            if (p.lse) p.lse[((size_t)b * p.n_sent + seg_sent[s]) * S_pad + r] = l;
          }
        }
      }
      __syncthreads();
      if (sweep == 0) continue;          // statistics sweep of a multi-tile sentence: next sub-tile
    }

    GLR_STAMP(2);
    // ================= P2: a1, e2 from the scores in registers; LDS image =================
    // (word-row loop outermost: the per-word scalars are live for one row at a time)
    float zq[16], dq[16];
    if (wactive) {
      // a lane's 16 word rows increase with q, so their sentence ids form runs: the per-(sentence, region)
      // log-sum-exp is (re)loaded only when the run changes
      int cur = -2;
      float lcur[3] = {0.f, 0.f, 0.f};
      float gcur[3] = {0.f, 0.f, 0.f};     // bwd: gradient of the word-mean attention row / words in the sentence
      // bwd: gradient of the attention map of the diagonal pair (attention-supervision loss), per (word, region)
      const bool has_dmap = BWD && AUX && p.dattn != nullptr;
      const int dw0 = has_dmap ? diag[0] : 0, dn = has_dmap ? diag[1] : 0;
      const int sout = p.S_eff - p.strip;
      const float* dmap = has_dmap ? p.dattn + p.attn_off[p.img_offset + b] + (size_t)wbase * sout - p.strip : nullptr;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        const int sg = wseg[word];
        const bool in_diag = has_dmap && word >= dw0 && word < dw0 + dn;
        float zi = 0.f, be = 0.f, al = 0.f;
        if (BWD) { zi = w_zi[word]; be = w_be[word]; al = w_al[word]; }
        if (sg != cur && sg >= 0) {
          cur = sg;
          const int sent = seg_sent[sg];
          const float ninv = 1.f / (float)(nsub > 1 ? long_n : seg_n[sg]);
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int region = min((wg + 4 * j) * 32 + l31, S_pad - 1);
            if (BWD) {
              lcur[j] = p.lse[((size_t)b * p.n_sent + sent) * S_pad + region];
              if (AUX && p.damean != nullptr) gcur[j] = p.damean[((size_t)b * p.n_sent + sent) * S_pad + region] * ninv;
            } else {
              lcur[j] = (nsub > 1) ? mrun[region] : sc[sg * SCP + region];
            }
          }
        }
        float zacc = 0.f, dacc = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int blk = wg + 4 * j;
          if (GLR_BLK_OK(blk)) {
            const int region = blk * 32 + l31;
            // branch-free: invalid (empty slot / padded region) elements are zeroed
            const bool ok = sg >= 0 && region < p.S_eff;
            const float a1 = ok ? __expf(acc[j][q] - lcur[j]) : 0.f;
            const float e2 = ok ? __expf(p.temp1 * a1) : 0.f;
            if (BWD) {
              // da2 = (alpha s - beta u) + g: the accumulator starts at -(alpha s + g), P3 adds beta u
              const float a2 = e2 * zi;
              O::from_f32(img + word * IMP + region * ESZ, be * a2);
              a1r[j][q] = a1;
              if (AUX) {
                float ge = gcur[j];
                if (in_diag && ok && region >= p.strip) ge += dmap[(size_t)(word - dw0) * sout + region];
                acc[j][q] = -al * acc[j][q] - (ok ? ge : 0.f);
                zacc += a2 * ge;                 // kappa gains sum_r a2 g  (softmax-over-regions backward)
              } else {
                acc[j][q] = -al * acc[j][q];
              }
            } else {
              O::from_f32(img + word * IMP + region * ESZ, e2);
              const float e2r = ESZ == 4 ? e2 : bf2f(f2bf(e2));        // as the MFMA will see it
              zacc += e2r;
              dacc += e2r * acc[j][q];
              acc[j][q] = 0.f;
            }
          }
        }
        zq[q] = zacc;
        dq[q] = dacc;
      }
    }
    if (!BWD) {
      // region sums: lanes 15/31/47/63 hold the totals of their 16-lane row -> 8 partials per word
      const int rslot = wg * 2 + ((lane >> 4) & 1);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float z = row_sum16(zq[q]), d = row_sum16(dq[q]);
        if ((lane & 15) == 15 && wactive) {
          const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          red[(0 * 8 + rslot) * TW + word] = z;
          red[(1 * 8 + rslot) * TW + word] = d;
        }
      }
    } else if (AUX && (p.damean != nullptr || p.dattn != nullptr)) {
      const int rslot = wg * 2 + ((lane >> 4) & 1);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float z = row_sum16(zq[q]);
        if ((lane & 15) == 15 && wactive) {
          const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          red[(1 * 8 + rslot) * TW + word] = z;          // rows 8..15 of red: free in the backward kernel
        }
      }
    }
    __syncthreads();        // image complete (and the score tile is dead: the ring may be reused)
    if (BWD && AUX && (p.damean != nullptr || p.dattn != nullptr) && tid < TW) {
      float kg = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) kg += red[(8 + k) * TW + tid];
      w_ka[tid] += kg;      // read by P4 behind the barriers of the P3 stream
    }

    GLR_STAMP(3);
    // ================= P3: acc[w, r] (+)= image . G^T =================
    stream_gemm<O, true>(acc, acc, wm * 32, 0, ring, buf2, nullptr, 0, gram_b, rowbytes2, S_pad, nch2, img, IMP, wave, lane, wm, wg,
                         nrb, tw);

    GLR_STAMP(4);
    if (BWD && p.baout != nullptr && sweep == 1) {
      // third output: the operand image beta a2 (rows >= tw of the tile are zero)
      const int rowb = S_pad * ESZ, ppr = rowb >> 4;
      for (int i = tid; i < TW * ppr; i += NTHR) {
        const int row = i / ppr, pc = i % ppr;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < tw) v = *reinterpret_cast<const uint4*>(img + row * IMP + pc * 16);
        *reinterpret_cast<uint4*>(p.baout + ((size_t)b * p.n_slots + (size_t)tile * TW + row) * rowb + pc * 16) = v;
      }
    }
    if (!BWD) {
      // |c~|^2 = sum_r e2[w, r] * u~[w, r]
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        float v = 0.f;
        if (wactive) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int blk = wg + 4 * j;
            if (GLR_BLK_OK(blk)) v += O::to_f32(img + word * IMP + (blk * 32 + l31) * ESZ) * acc[j][q];
          }
        }
        v = row_sum16(v);
        if ((lane & 15) == 15 && wactive) red[(2 * 8 + wg * 2 + ((lane >> 4) & 1)) * TW + word] = v;
      }
      __syncthreads();

      // ================= P4 (forward): cosine, per-sentence aggregate =================
      if (tid < tw) {
        float z = 0.f, dd = 0.f, nn = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          z += red[(0 * 8 + k) * TW + tid];
          dd += red[(1 * 8 + k) * TW + tid];
          nn += red[(2 * 8 + k) * TW + tid];
        }
        float cosv = 0.f, nc2 = 0.f;
        if (z > 0.f) {
          const float iz = 1.f / z;
          nc2 = fmaxf(nn, 0.f) * iz * iz;                      // |c_w|^2
          const float den = fmaxf(p.tnorm[(size_t)tile * TW + tid] * sqrtf(nc2), p.eps);
          cosv = dd * iz / den;
        }
        zsum[tid] = z;
        exs[tid] = __expf(p.temp2 * cosv);
        if (p.wstat) {
          float* ws = p.wstat + ((size_t)b * p.n_slots + (size_t)tile * TW + tid) * WSTAT;
          ws[0] = z; ws[1] = cosv; ws[2] = nc2; ws[3] = 0.f;
        }
      }
      __syncthreads();
      if (p.amean != nullptr && tid < S_pad) {
        // word-mean attention row A[r] = mean_w a2[w, r] of every sentence of the tile (aux regularisers,
        // gloria_loss.py:131-139); a multi-tile sentence accumulates across its sub-tiles in srun
        const int r = tid;
        for (int s = 0; s < nseg; ++s) {
          const int w0 = seg_w0[s], n = seg_n[s];
          float a = 0.f;
          for (int w = 0; w < n; ++w) a += O::to_f32(img + (w0 + w) * IMP + r * ESZ) / zsum[w0 + w];
          int ntot = n;
          bool emit = true;
          if (nsub > 1) {
            if (sub > 0) a += srun[r];
            srun[r] = a;
            emit = (sub == nsub - 1);
            ntot = long_n;
          }
          if (emit) p.amean[((size_t)b * p.n_sent + seg_sent[s]) * S_pad + r] = r < p.S_eff ? a / (float)ntot : 0.f;
        }
      }
      if (tid < nseg) {
        const int w0 = seg_w0[tid], n = seg_n[tid];
        float v = 0.f;
        if (p.agg == GLR_AGG_MAX) {
          for (int w = 0; w < n; ++w) v = fmaxf(v, exs[w0 + w]);
        } else {
          for (int w = 0; w < n; ++w) v += exs[w0 + w];
        }
        bool emit = true;
        int ntot = n;
        if (nsub > 1) {        // accumulate across the sub-tiles of a multi-tile sentence (tid == 0 only)
          v = (p.agg == GLR_AGG_MAX) ? fmaxf(v, aggv[0]) : v + aggv[0];
          aggv[0] = v;
          emit = (sub == nsub - 1);
          ntot = long_n;
        }
        if (p.agg == GLR_AGG_MEAN) v /= (float)ntot;
        const int sent = seg_sent[tid];
        if (emit && (!p.pair_only || sent == p.img_offset + b))
          p.sim[(size_t)b * p.ld_sim + sent] = p.temp3 * __logf(v);
      }
      // attention map of the diagonal pair: a2[w, r] = e2[w, r] / Z_w, no-attention column stripped
      const int dw0 = diag[0], dn = diag[1];
      if (p.attn != nullptr && dn > 0) {
        const int sout = p.S_eff - p.strip;
        float* out = p.attn + p.attn_off[p.img_offset + b] + (size_t)wbase * sout;
        for (int idx = tid; idx < dn * sout; idx += NTHR) {
          const int w = idx / sout, r = idx % sout + p.strip;
          out[idx] = O::to_f32(img + (dw0 + w) * IMP + r * ESZ) / zsum[dw0 + w];
        }
      }
    } else {
      // ================= P4 (backward) =================
      // acc = beta*u - alpha*s = -da2.  softmax-over-regions backward needs only kappa_w;
      // softmax-over-words backward needs rho[r, sentence] = sum_w a1*da1 (LDS atomics).
      float* rho = (nsub > 1) ? srun : reinterpret_cast<float*>(smem);       // [nseg][S_pad]
      if (nsub == 1) {
        for (int i = tid; i < nseg * S_pad; i += NTHR) rho[i] = 0.f;
        __syncthreads();
      }
      GLR_STAMP(5);
      // rho[r, sentence] += sum over this lane's rows of the sentence of a1*da1: the rows of a sentence
      // are a run along q, so the sum is kept in registers and ONE LDS atomic is issued per run
      // (16 same-address atomics per lane serialise in the LDS atomic unit: 76k -> cycles measured)
      {
        int cur = -1;
        float run[3] = {0.f, 0.f, 0.f};
        const bool do_rho = (nsub == 1 || sweep == 0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          const int sg = wseg[word];
          const int rrow = (nsub > 1) ? 0 : sg;
          const float zi = w_zi[word], ka = w_ka[word];
          if (sg >= 0 && rrow != cur) {
            if (cur >= 0 && do_rho) {
#pragma unroll
              for (int j = 0; j < 3; ++j)
                if (GLR_BLK_OK(wg + 4 * j)) atomicAdd(&rho[cur * S_pad + (wg + 4 * j) * 32 + l31], run[j]);
            }
            cur = rrow;
            run[0] = run[1] = run[2] = 0.f;
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int blk = wg + 4 * j;
            if (GLR_BLK_OK(blk)) {
              const int region = blk * 32 + l31;
              const float a1 = a1r[j][q];
              const bool ok = sg >= 0 && region < p.S_eff;
              const float a2 = __expf(p.temp1 * a1) * zi;
              const float da1 = ok ? p.temp1 * a2 * (-acc[j][q] - ka) : 0.f;
              run[j] += ok ? a1 * da1 : 0.f;
              acc[j][q] = da1;
            }
          }
        }
        if (cur >= 0 && do_rho) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
            if (GLR_BLK_OK(wg + 4 * j)) atomicAdd(&rho[cur * S_pad + (wg + 4 * j) * 32 + l31], run[j]);
        }
      }
      __syncthreads();
      GLR_STAMP(6);
      if (sweep == 1) {
        // outputs X = ds + alpha*a2 and a2, staged through the (now free) image region so that every
        // global store is a 16-byte piece of a full row; rows >= tw of the tile are zero
        const int rowb = S_pad * ESZ;                   // bytes per output row
        const int ppr = rowb >> 4;                      // 16-byte pieces per row
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int word = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
            const int sg = wseg[word];
            const int rrow = (nsub > 1) ? 0 : max(sg, 0);
            const float zi = w_zi[word], al = w_al[word];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const int blk = wg + 4 * j;
              if (GLR_BLK_OK(blk) && wactive) {
                const int region = blk * 32 + l31;
                const bool ok = sg >= 0 && region < p.S_eff;
                const float a1 = a1r[j][q];
                const float a2 = ok ? __expf(p.temp1 * a1) * zi : 0.f;
                float v = a2;
                if (which == 0) {
                  const float ds = a1 * (acc[j][q] - rho[rrow * S_pad + region]);
                  v = ok ? ds + al * a2 : 0.f;
                }
                O::from_f32(img + word * IMP + region * ESZ, v);
              }
            }
          }
          wg_barrier();
          GLR_STAMP(7 + 2 * which);
          unsigned char* dst = which == 0 ? p.xout : p.aout;
          for (int i = tid; i < TW * ppr; i += NTHR) {
            const int row = i / ppr, pc = i % ppr;
            const size_t slot = (size_t)tile * TW + row;
            const size_t grow = which == 0 ? (slot * p.B_img + b) : ((size_t)b * p.n_slots + slot);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < tw) v = *reinterpret_cast<const uint4*>(img + row * IMP + pc * 16);
            *reinterpret_cast<uint4*>(dst + grow * rowb + pc * 16) = v;
          }
          wg_barrier();      // LDS reads done; the global stores stay in flight (no vmcnt drain)
          GLR_STAMP(8 + 2 * which);
        }
      }
    }
    GLR_STAMP(11);
  }  // sub / sweep loops
}

// ------------------------------------------------------------------------------------------
// Forward for a PAIR of tiles, wave-owned words (the production forward for the 384-region shape, bf16).
//
// One 512-thread workgroup = one image x a PAIR of 64-slot word tiles: vt[b] and gram[b] pass through LDS once per 128
// words (the streams are bound by the L2 -> LDS path, ~48 B/clk/CU, so bytes per word decide their time).  The eight
// waves are mapped  wave -> (tile t = wave & 1, region group wg = wave >> 1): a wave holds ALL 64 word slots of its tile
// (two 32-word MFMA blocks, acc0 / acc1) for its three region blocks.  The word softmax (a1 = softmax over the
// words of a sentence, per region) is then private to the wave: every (sentence, region column) statistic is
// combined between the two lane halves of ONE wave, through a table only that wave touches.  No workgroup barrier
// and no finalize loop between the end of the score stream and the completed e2 image.
//
// Rows.  Lane half h owns the slots w with ((w >> 2) & 1) == h: 32 rows in word order, row k < 16 = acc0[.][k],
// k >= 16 = acc1[.][k - 16].  A sentence is a run of rows; where runs start / end is the same for all lanes of a
// half and comes from the planner as bit masks (glr_plan_rowflags), so the fully unrolled row loops branch on
// SCALAR bits and do per-lane work only at run boundaries:
//   pass 1  running max; at a run end  plain store -> mx[lane half][sentence][region]      (log2 units)
//   pass 2  running sum of exp2(s log2e - max); at a run end plain store -> sm[lane half][sentence][region]
//           (one writer per entry; readers combine the two halves in a fixed order: bitwise reproducible)
//   P2      at a run start lse = mx + log2(sm) (the owner half also stores it for the backward pass); per element
//           a1 = exp2(s log2e - lse), e2 = exp2(temp1 log2e a1) -> bf16 image [word][region]; dot~ by DPP row sums
// Z_w = sum_r e2[w, r] is NOT reduced on the vector ALU: the packed Gram operand carries ones in row S_pad - 1
// (a padded region: columns r < S_eff), so the second MFMA contraction leaves Z_w in output column S_pad - 1.
// A sentence of 65..128 words owns both tiles: its two tiles keep separate table rows (row = tile) that are
// combined in a fixed order behind a workgroup barrier (the only case with barriers inside the statistics).
// LDS: [0, 2*IMG) images (earlier: P1 ring) | [2*IMG, +48 KiB) mx / sm half tables, then the 2-deep P3 ring | small.

template <typename O>
__global__ void __launch_bounds__(NTHR) k_local_attn_pw(LaParams p) {
  constexpr int ESZ = O::ESZ, CB = CHB;
  constexpr int SP = GLR_MAX_SPAD;
  constexpr int NRB = SP / 32;
  constexpr int IMP = SP * ESZ + 16;
  constexpr int IMG = TW * IMP;
  constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = wave & 1, wg = wave >> 1;
  const int l31 = lane & 31, h = lane >> 5;

  // Block -> (image, item).  Blocks with equal blockIdx % 8 share an XCD (speed only).  Per XCD the blocks walk
  // groups of `img_block` images x all items, images innermost: the XCD's concurrently resident workgroups then
  // share img_block images (vt + gram: 885 KB each) AND a few word-tile pairs (196 KB each) in the 4 MiB L2.
  const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
  const int ib = p.img_block;
  const int grp = qq / (ib * p.n_items), rem = qq - grp * (ib * p.n_items);
  const int b = (grp * ib + rem % ib) * 8 + xcd;
  if (b >= p.B_img) return;
  GLR_STAMP2(0);
  const int tile0 = p.item_tile[rem / ib];
  const int D = p.D;

  unsigned char* ring = smem;
  unsigned char* img0 = smem;
  // statistics tables, one writer per entry (plain stores: LDS float atomics cost ~50 LDS cycles per wave
  // instruction and stall every other LDS access of the CU): [lane half][sentence][region]
  float* mx = reinterpret_cast<float*>(smem + p.off_img);        // [2][PW_MAXSEG][SP] run maxima, log2 units
  float* sm = mx + 2 * PW_MAXSEG * SP;                           // [2][PW_MAXSEG][SP] run sums of exp2
  constexpr int HT = PW_MAXSEG * SP;                             // floats from one half's table to the other's
  unsigned char* ring3 = smem + p.off_img;
  signed char* wsegb = reinterpret_cast<signed char*>(smem + p.off_small);   // [2 * TW] sentence index in the pair, -1 = empty
  int* seg_w0 = reinterpret_cast<int*>(wsegb + 2 * TW);
  int* seg_n = seg_w0 + PW_MAXSEG;
  int* seg_sent = seg_n + PW_MAXSEG;
  int* misc = seg_sent + PW_MAXSEG;                              // [1..2] diagonal w0, n; [8..9] long-pair partials; [16..79] descriptor
  float* tnl = reinterpret_cast<float*>(misc + 80);              // [2 * TW] word norms
  float* zsum = tnl + 2 * TW;                                    // [2 * TW]
  float* dsum = zsum + 2 * TW;                                   // [2 * TW]
  float* red = dsum + 2 * TW;                                    // [2 tiles][2][8][TW]

  const size_t rowbytes1 = (size_t)D * ESZ, rowbytes2 = (size_t)SP * ESZ;
  const unsigned char* vt_b = p.vt + (size_t)b * SP * rowbytes1;
  const unsigned char* gram_b = p.gram + (size_t)b * SP * rowbytes2;

  // everything about the pair comes from ONE 256-byte descriptor (coalesced; the segment tables used to cost three
  // dependent global round trips before the stream could start)
  int* dsc = misc + 16;                                          // [64] LDS copy of the pair descriptor
  if (tid < 64) dsc[tid] = p.pair_desc[(size_t)(rem / ib) * 64 + tid];
  if (tid < 2 * TW) {
    wsegb[tid] = -1;
    tnl[tid] = p.tnorm[(size_t)tile0 * TW + tid];
  }
  if (tid < 3) misc[tid] = 0;
  __syncthreads();
  const int NS = dsc[0];
  const bool long_pair = dsc[1] != 0;
  if (tid < NS) {
    const int sent = dsc[8 + tid], w0 = dsc[16 + tid], n = dsc[24 + tid];
    seg_sent[tid] = sent;
    seg_w0[tid] = w0;
    seg_n[tid] = n;
    for (int w = 0; w < n; ++w) wsegb[w0 + w] = (signed char)tid;
    if (sent == p.img_offset + b) { misc[1] = w0; misc[2] = n; }
  }
  // ================= P1 (both tiles, one stream of vt[b]) =================
  f32x16 acc0[3], acc1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[j][q] = 0.f; acc1[j][q] = 0.f; }
  __syncthreads();
  GLR_STAMP2(1);
  if (!GLR_SKIP(1))
  stream_gemm<O, false, 2>(acc0, acc1, t * TW, 32 * CB, ring, (2 * TW + SP) * CB, p.tp + (size_t)tile0 * TW * rowbytes1,
                           rowbytes1, vt_b, rowbytes1, SP, (int)(rowbytes1 / CB), nullptr, 0, wave, lane, 0, wg, NRB, TW);
  GLR_STAMP2(2);

  // run boundaries of this wave's tile (scalar: same for every lane of a half); read from the LDS copy of the
  // descriptor after the stream so that they are not carried (and spilled) through it
  const int* fl = dsc + 32 + 8 * t;
  const unsigned ST0 = __builtin_amdgcn_readfirstlane(fl[0]), ST1 = __builtin_amdgcn_readfirstlane(fl[1]),
                 LA0 = __builtin_amdgcn_readfirstlane(fl[2]), LA1 = __builtin_amdgcn_readfirstlane(fl[3]);
  const unsigned STANY = ST0 | ST1, LAANY = LA0 | LA1;
  const unsigned STh = h ? ST1 : ST0, LAh = h ? LA1 : LA0;
  // a wave-uniform bit test the compiler must keep as a SCALAR branch: without the opaque copy it folds the test
  // into the per-lane predicate below it and every row pays an exec-mask sequence
// (expected false: run boundaries are rare, so the boundary blocks are laid out of line and the common path falls
// through instead of taking a branch over them at every row)
#define GLR_SBIT(mask, k) __builtin_expect(([&] { unsigned b_ = ((mask) >> (k)) & 1u; asm volatile("" : "+s"(b_)); return b_ != 0; }()), 0)

  // sentence ids of this lane's 32 rows: row k -> slot (k >> 4) * 32 + 8 * ((k & 15) >> 2) + 4 h + (k & 3); the
  // four rows of a group are four consecutive bytes of the slot table
  int sgp[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) sgp[g] = *reinterpret_cast<const int*>(wsegb + t * TW + (g >> 2) * 32 + 4 * h + 8 * (g & 3));
#define GLR_SGK(k) ((sgp[(k) >> 2] << (24 - 8 * ((k) & 3))) >> 24)
  const int rbase = wg * 32 + l31;              // this lane's region in block j: rbase + 128 * j
  const float t1l = p.temp1 * LOG2E;
  const int rslot = wg * 2 + ((lane >> 4) & 1);
  // the bf16-rounded e2 of both word blocks stay in registers (two per dword) for the |c|^2 sums of P4
  unsigned e2k0[3][8], e2k1[3][8];

  // Table rows: a sentence's index in the pair.  The ONE sentence of a long pair (65..128 words, both tiles) uses
  // row = tile instead and its two tiles are combined behind workgroup barriers.  Readers therefore combine "their"
  // row with a second row: the other tile's (long pair) or a constant neutral row (-inf / 0) kept in the unused
  // half of `red` - one code path for both kinds (a specialised second copy pushed the kernel past the 64 KiB
  // instruction cache, and so did fat per-row boundary blocks: the combining of lane halves is done once per
  // sentence in two short rolled loops, fin1 / fin2, not at every run boundary).
  float* zneg = red + 8 * TW;                   // [SP] -inf   (rows 8..15 of tile 0's partial table: unused here)
  float* zero = red + 16 * TW + 8 * TW;         // [SP] 0      (rows 8..15 of tile 1's)
  if (h == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { zneg[rbase + 128 * j] = -INFINITY; zero[rbase + 128 * j] = 0.f; }
  }
  const float* mx2 = (long_pair ? mx + SP : zneg) + rbase;      // second row of the combined maxima
  const float* sm2 = (long_pair ? sm + SP : zero) + rbase;      // second row of the sums (half 0; half 1 at + HT2)
  const int HT2 = long_pair ? HT : 0;
  float* lt = mx + HT;                          // [PW_MAXSEG][SP] lse, log2 units (half-1 maxima are dead after fin1)
  const int nrow = long_pair ? 2 : NS;
  {
    // this wave's table entries - the rows of ITS tile's sentences (the other tile's waves own the same columns),
    // its columns: every lane half clears its own half tables (a sentence may have no row in a half)
    {
      float* tm = mx + h * HT + rbase;
      float* ts = sm + h * HT + rbase;
      for (int s2 = 0; s2 < nrow; ++s2) {
        if ((long_pair ? s2 : (seg_w0[s2] >> 6)) != t) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) { tm[s2 * SP + 128 * j] = -INFINITY; ts[s2 * SP + 128 * j] = 0.f; }
      }
    }
    if (!GLR_SKIP(2)) {
    // ---- pass 1: run maxima (v_max_f32 by hand: fmaxf() canonicalises both inputs first, three instructions)
    {
      float rm[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
        const int q = k & 15;
#pragma unroll
        for (int j = 0; j < 3; ++j) asm("v_max_f32 %0, %1, %2" : "=v"(rm[j]) : "v"(rm[j]), "v"(acc[j][q]));
        if (GLR_SBIT(LAANY, k)) {
          const bool mine = (LAh >> k) & 1;
          if (mine) {
            float* dst = mx + h * HT + (long_pair ? t : GLR_SGK(k)) * SP + rbase;
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[128 * j] = rm[j] * LOG2E;
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) rm[j] = mine ? -INFINITY : rm[j];
        }
      }
    }
    if (long_pair) __syncthreads();             // the other tile's maxima of the spanning sentence
    // fin1: maxima of both lane halves -> half-0 table, sentences split between the halves.  (Long pair: the waves
    // of both tiles own these columns and write identical values; max is idempotent, so the overlap is harmless.)
    for (int s2 = h; s2 < nrow; s2 += 2) {
      if (!long_pair && (seg_w0[s2] >> 6) != t) continue;
      float* e = mx + s2 * SP + rbase;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float m = e[128 * j];
        const float mb = e[HT + 128 * j];
        asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(mb));
        e[128 * j] = m;
      }
    }
    GLR_STAMP2(3);
    // ---- pass 2: run sums of exp2(s log2e - max)
    {
      float rs[3] = {0.f, 0.f, 0.f}, mc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
        const int q = k & 15;
        if (GLR_SBIT(STANY, k)) {
          const bool mine = (STh >> k) & 1;
          const float* src = mx + (long_pair ? 0 : max(GLR_SGK(k), 0)) * SP + rbase;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            float m = src[128 * j];
            const float m1 = mx2[128 * j];
            asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(m1));
            mc[j] = mine ? m : mc[j];
            rs[j] = mine ? 0.f : rs[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[j] += __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], LOG2E, -mc[j]));
        if (GLR_SBIT(LAANY, k)) {
          if ((LAh >> k) & 1) {
            float* dst = sm + h * HT + (long_pair ? t : GLR_SGK(k)) * SP + rbase;
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[128 * j] = rs[j];
          }
        }
      }
    }
    if (long_pair) __syncthreads();
    // fin2: lse = max + log2(sum of the halves (and of the second row)), fixed order; stored for the backward pass.
    // Long pair: one row (0) for the whole sentence, stored by the waves of tile 0.
    for (int s2 = h; s2 < (long_pair ? 1 : NS); s2 += 2) {
      if (!long_pair && (seg_w0[s2] >> 6) != t) continue;
      const float* em = mx + s2 * SP + rbase;
      const float* es = sm + s2 * SP + rbase;
      float* dst = (p.lse != nullptr && (!long_pair || t == 0))
                       ? p.lse + ((size_t)b * p.n_sent + seg_sent[s2]) * SP + rbase : nullptr;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float m = em[128 * j];
        const float m1 = mx2[128 * j];
        asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(m1));
        const float su = (es[128 * j] + es[HT + 128 * j]) + (sm2[128 * j] + sm2[HT2 + 128 * j]);
        const float l2 = m + __builtin_amdgcn_logf(su);            // v_log_f32 = log2
        lt[s2 * SP + rbase + 128 * j] = l2;
        if (dst != nullptr) dst[128 * j] = l2 * LN2;
      }
    }
    if (long_pair) __syncthreads();             // tile 1 reads the row tile 0's waves may still be writing
    }
    GLR_STAMP2(4);

    // ---- P2: a1, e2 from the scores in registers; LDS image; per-word dot~
    // Branch-free per element: padded regions (r >= S_eff) have zero vt rows and zero Gram columns, and the ones
    // row of the Gram operand only covers r < S_eff, so their e2 reaches neither u nor Z; empty word slots compute
    // finite garbage that no sentence ever reads.
    if (!GLR_SKIP(4)) {
      float lc[3] = {0.f, 0.f, 0.f};
      unsigned* a1out = p.a1buf == nullptr ? nullptr
                        : p.a1buf + (((size_t)b * p.a1_items + p.a1_base + rem / ib) * 8 + wave) * (2 * 3 * 8 * 64) + lane;
      unsigned char* imgw = img0 + t * IMG + (4 * h) * IMP + rbase * ESZ;   // + (blk * 32 + row(q)) * IMP + 128 * j * ESZ
      float* redt = red + t * 16 * TW + rslot * TW + 4 * h;                // + blk * 32 + row(q)
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        f32x16(&acc)[3] = blk == 0 ? acc0 : acc1;
        unsigned(&e2k)[3][8] = blk == 0 ? e2k0 : e2k1;
        float dq[16];                           // per-row partial dot~: reduced across lanes after the block (ILP)
        float a1e[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int k = blk * 16 + q;
          const int row = blk * 32 + (q & 3) + 8 * (q >> 2);
          if (GLR_SBIT(STANY, k)) {
            const bool mine = (STh >> k) & 1;
            const float* src = lt + (long_pair ? 0 : max(GLR_SGK(k), 0)) * SP + rbase;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const float l2 = src[128 * j];
              lc[j] = mine ? l2 : lc[j];
            }
          }
          float dacc = 0.f;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const float a1 = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[j][q], LOG2E, -lc[j]));
            if (a1out != nullptr) {
              // hand a1 to the backward (fp16 pairs of rows q, q + 1; one coalesced 256-byte store per wave instruction)
              // (clamped: an empty word slot sees a stale lse and may give inf, which the backward must never meet)
              float a1c;
              asm("v_min_f32 %0, 1.0, %1" : "=v"(a1c) : "v"(a1));
              if (q & 1) {
                unsigned pk;
                asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(pk) : "v"(a1e[j]), "v"(a1c));
                a1out[((blk * 3 + j) * 8 + (q >> 1)) * 64] = pk;
              } else {
                a1e[j] = a1c;
              }
            }
            const float e2 = __builtin_amdgcn_exp2f(t1l * a1);
            O::from_f32(imgw + row * IMP + 128 * j * ESZ, e2);
            const float e2r = ESZ == 4 ? e2 : bf2f(f2bf(e2));
            const unsigned eb = __float_as_uint(e2r);                      // low 16 bits are zero
            e2k[j][q >> 1] = (q & 1) ? (e2k[j][q >> 1] | eb) : (eb >> 16);
            dacc = __builtin_fmaf(e2r, acc[j][q], dacc);
          }
          dq[q] = dacc;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float d = row_sum16(dq[q]);
          if ((lane & 15) == 15) redt[blk * 32 + (q & 3) + 8 * (q >> 2)] = d;
        }
      }
    }
  }
#undef GLR_SBIT
  __syncthreads();                              // images complete; the tables are dead: the P3 ring takes their place
  if (tid < 2 * TW) {
    const float* redt = red + (tid >> 6) * 16 * TW + (tid & 63);
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += redt[k * TW];
    dsum[tid] = d;
  }
  GLR_STAMP2(5);

  // ================= P3 (both word blocks, one stream of gram[b]); first MFMA of every chain starts from zero ====
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[j][q] = 0.f; acc1[j][q] = 0.f; }
  if (!GLR_SKIP(8))
  stream_gemm<O, true, 2, 2>(acc0, acc1, 0, 32 * IMP, ring3, SP * CB, nullptr, 0, gram_b, rowbytes2, SP,
                            (int)(rowbytes2 / CB), img0 + t * IMG, IMP, wave, lane, 0, wg, NRB, TW);
  GLR_STAMP2(6);

  // ================= P4: Z from the ones row, |c|^2, cosine, per-sentence aggregate, maps =================
  if (!GLR_SKIP(16)) {
  if (wg == 3 && l31 == 31) {                   // output column SP - 1 = sum_r<S_eff e2[w, r]
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
      const int q = k & 15;
      zsum[t * TW + (k >> 4) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h] = acc[2][q];
    }
  }
  {
    const float ok2 = (rbase + 256 < p.S_eff) ? 1.f : 0.f;      // padded columns (incl. the Z column) live in block 2 only
    float* redt = red + t * 16 * TW + rslot * TW + 4 * h;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
      const unsigned(&e2k)[3][8] = k < 16 ? e2k0 : e2k1;
      const int q = k & 15;
      const int row = (k >> 4) * 32 + (q & 3) + 8 * (q >> 2);
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned u = e2k[j][q >> 1];
        const float e = __uint_as_float((q & 1) ? (u & 0xffff0000u) : (u << 16));
        v += (j == 2 ? ok2 * e : e) * acc[j][q];
      }
      v = row_sum16(v);
      if ((lane & 15) == 15) redt[row] = v;
    }
  }
  }
  __syncthreads();
  GLR_STAMP2(7);
  if (tid < 2 * TW) {            // waves 0 / 1 = tile A / B, lane = word slot
    const float* redt = red + wave * 16 * TW + lane;
    float nn = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) nn += redt[k * TW];
    const float z = zsum[tid], dd = dsum[tid];
    float cosv = 0.f, nc2 = 0.f;
    if (z > 0.f) {
      const float iz = 1.f / z;
      nc2 = fmaxf(nn, 0.f) * iz * iz;
      const float den = fmaxf(tnl[tid] * sqrtf(nc2), p.eps);
      cosv = dd * iz / den;
    }
    if (p.wstat) {
      float* ws = p.wstat + ((size_t)b * p.n_slots + (size_t)tile0 * TW + tid) * WSTAT;
      ws[0] = z; ws[1] = cosv; ws[2] = nc2; ws[3] = 0.f;
    }
    // per-sentence aggregate: segmented inclusive scan along the lanes (sentences are lane runs),
    // fixed order -> bitwise reproducible
    const int sg = wsegb[tid];
    float v = __expf(p.temp2 * cosv);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float o = __shfl_up(v, off, 64);
      const int so = __shfl_up(sg, off, 64);
      if (lane >= off && so == sg) v = (p.agg == GLR_AGG_MAX) ? fmaxf(v, o) : v + o;
    }
    const int snext = __shfl_down(sg, 1, 64);
    if (sg >= 0 && (lane == 63 || snext != sg)) {
      if (long_pair) {
        reinterpret_cast<float*>(misc)[8 + wave] = v;      // this tile's part of the spanning sentence
      } else {
        if (p.agg == GLR_AGG_MEAN) v /= (float)seg_n[sg];
        p.sim[(size_t)b * p.ld_sim + seg_sent[sg]] = p.temp3 * __logf(v);
      }
    }
  }
  if (long_pair) {
    __syncthreads();
    if (tid == 0) {
      const float* part = reinterpret_cast<const float*>(misc) + 8;
      float v = (p.agg == GLR_AGG_MAX) ? fmaxf(part[0], part[1]) : part[0] + part[1];
      if (p.agg == GLR_AGG_MEAN) v /= (float)seg_n[0];
      p.sim[(size_t)b * p.ld_sim + seg_sent[0]] = p.temp3 * __logf(v);
    }
  }
  const int dw0 = misc[1], dn = misc[2];
  if (p.attn != nullptr && dn > 0) {            // the diagonal sentence lies inside one tile, or spans both (long pair)
    const int sout = p.S_eff - p.strip;
    float* out = p.attn + p.attn_off[p.img_offset + b];
    for (int idx = tid; idx < dn * sout; idx += NTHR) {
      const int w = dw0 + idx / sout, r = idx % sout + p.strip;
      out[idx] = O::to_f32(img0 + (w >> 6) * IMG + (w & 63) * IMP + r * ESZ) / zsum[w];
    }
  }
  if (p.amean != nullptr && tid < SP) {
    // word-mean attention row A[r] = mean_w a2[w, r] of every sentence of the pair (aux regularisers,
    // gloria_loss.py:131-139), from the e2 images and the per-word Z
    const int r = tid;
    for (int s2 = 0; s2 < NS; ++s2) {
      const int w0 = seg_w0[s2], n = seg_n[s2];
      float a = 0.f;
      for (int w = w0; w < w0 + n; ++w) a += O::to_f32(img0 + (w >> 6) * IMG + (w & 63) * IMP + r * ESZ) / zsum[w];
      p.amean[((size_t)b * p.n_sent + seg_sent[s2]) * SP + r] = r < p.S_eff ? a / (float)n : 0.f;
    }
  }
  GLR_STAMP2(8);
#undef GLR_SGK
}

// ------------------------------------------------------------------------------------------
// Backward for a PAIR of tiles, wave-owned words: the forward pair kernel's decomposition (same descriptor, same
// streams, same lane -> (word row, region) mapping) applied to autograd through gloria_loss.py:19-63, 150-164.
//   set-up  per-word scalars (alpha, beta, kappa, 1/Z: float4 per slot) from dsim and the forward's statistics;
//           the lse rows of the pair's sentences -> LDS (log2 units); a1 of the forward pair kernels
//           (LaParams::a1buf, fp16 pairs in this kernel's own register order) -> registers.  There is no score
//           stream: the score itself, needed for -alpha s, is s = lse + log(a1).
//   P2      a2 = exp2(temp1 log2e a1) / Z; image = bf16(beta a2); acc = -alpha s;
//           a1 stays in registers as fp16 pairs (48 registers; fp32 copies do not fit beside 96 accumulators)
//   P3      acc += image . G^T = beta u - alpha s = -da2      (stream of gram[b])
//   A       da1 = temp1 a2 (da2 - kappa); run sums of a1 da1 per (sentence, region) -> one-writer half tables
//           (no LDS atomics); acc = a1 da1 + alpha a2; image = bf16(a2) -> aout (16-byte row stores)
//   B       rho = fixed-order sum of the half tables (and of the other tile's row for a spanning sentence);
//           X = acc - a1 rho -> image -> xout
// Optional third output baout = the P3 operand image beta a2 (saves the caller an elementwise pass in front of the
// P = (beta a2)^T a2 GEMM).  Empty word slots have zero scalars: their rows of every output are exact zeros.
// AUX: the extra gradient inputs `damean` (word-mean attention rows: regularisers) and `dattn` (diagonal
// attention maps: attention supervision), g[w, r] = damean[b, sentence(w), r] / n_words (+ dattn[w, r] on the diagonal
// pair): da2 gains g, i.e. the accumulator starts at -(alpha s + g), and kappa_w gains sum_r a2[w, r] g[w, r].  The
// damean rows of the pair's sentences are parked in LDS beside the lse rows.
template <typename O, bool AUX>
__global__ void __launch_bounds__(NTHR) k_local_attn_pw_bwd(LaParams p) {
  constexpr int ESZ = O::ESZ, CB = CHB;
  constexpr int SP = GLR_MAX_SPAD;
  constexpr int NRB = SP / 32;
  constexpr int IMP = SP * ESZ + 16;
  constexpr int IMG = TW * IMP;
  constexpr int PPR = SP * ESZ / 16;                              // 16-byte pieces per output row
  constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
  constexpr int LT_OFF = NBUF * (2 * TW + SP) * CB;               // lse table: past the images and the tables at off_img
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = wave & 1, wg = wave >> 1;
  const int l31 = lane & 31, h = lane >> 5;

  const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
  const int ib = p.img_block;
  const int grp = qq / (ib * p.n_items), rem = qq - grp * (ib * p.n_items);
  const int b = (grp * ib + rem % ib) * 8 + xcd;
  if (b >= p.B_img) return;
  GLR_STAMP2(0);
  const int tile0 = p.item_tile[rem / ib];
  unsigned a1k0[3][8], a1k1[3][8];                                // a1 as fp16 pairs (rows q, q + 1)
  {
    // 48 coalesced dword loads per lane, in flight behind the whole set-up
    const unsigned* a1in = p.a1buf + (((size_t)b * p.a1_items + p.a1_base + rem / ib) * 8 + wave) * (2 * 3 * 8 * 64) + lane;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) { a1k0[j][i] = a1in[(j * 8 + i) * 64]; a1k1[j][i] = a1in[((3 + j) * 8 + i) * 64]; }
  }

  unsigned char* img0 = smem;
  float* rh = reinterpret_cast<float*>(smem + p.off_img);        // [2][PW_MAXSEG][SP] run sums of a1 da1 (after P3)
  constexpr int HT = PW_MAXSEG * SP;
  unsigned char* ring3 = smem + p.off_img;
  float* lt = reinterpret_cast<float*>(smem + LT_OFF);           // [PW_MAXSEG][SP] lse, log2 units (P2 only)
  signed char* wsegb = reinterpret_cast<signed char*>(smem + p.off_small);
  int* seg_w0 = reinterpret_cast<int*>(wsegb + 2 * TW);
  int* seg_n = seg_w0 + PW_MAXSEG;
  int* seg_sent = seg_n + PW_MAXSEG;
  int* misc = seg_sent + PW_MAXSEG;                              // [16..79] descriptor
  float4* w4 = reinterpret_cast<float4*>(misc + 80);             // [2 * TW] (1/Z, beta, alpha, kappa) per word slot
  float* zero = reinterpret_cast<float*>(w4 + 2 * TW);           // [SP] neutral second table row
  [[maybe_unused]] float* kred = zero + SP;                      // AUX: [8][2 * TW] partial sums of a2 g per word
  [[maybe_unused]] float* gt = reinterpret_cast<float*>(smem + p.off_img);   // AUX: [PW_MAXSEG][SP] damean / n (P2 only)

  const size_t rowbytes2 = (size_t)SP * ESZ;
  const unsigned char* gram_b = p.gram + (size_t)b * SP * rowbytes2;

  int* dsc = misc + 16;
  if (tid < 64) dsc[tid] = p.pair_desc[(size_t)(rem / ib) * 64 + tid];
  // slot-indexed statistics do not depend on the descriptor: first round trip
  float4 ws = make_float4(0.f, 0.f, 0.f, 0.f);
  float tn = 0.f;
  if (tid < 2 * TW) {
    wsegb[tid] = -1;
    const size_t slot = (size_t)tile0 * TW + tid;
    ws = *reinterpret_cast<const float4*>(p.wstat + ((size_t)b * p.n_slots + slot) * WSTAT);
    tn = p.tnorm[slot];
  }
  if (tid < SP) zero[tid] = 0.f;
  if (tid < 3) misc[tid] = 0;
  __syncthreads();
  const int NS = dsc[0];
  const bool long_pair = dsc[1] != 0;
  if (tid < NS) {
    const int sent = dsc[8 + tid], w0 = dsc[16 + tid], n = dsc[24 + tid];
    seg_sent[tid] = sent;
    seg_w0[tid] = w0;
    seg_n[tid] = n;
    for (int w = 0; w < n; ++w) wsegb[w0 + w] = (signed char)tid;
    if (AUX && sent == p.img_offset + b) { misc[1] = w0; misc[2] = n; }
  }
  __syncthreads();
  // second round trip: dsim / sim of the slot's sentence, and the
  // lse rows of the pair's sentences (6 coalesced values per thread)
  float gsim = 0.f, vsim = 0.f;
  int sgw = -1;
  if (tid < 2 * TW) {
    sgw = wsegb[tid];
    if (sgw >= 0) {
      const size_t o = (size_t)b * p.ld_sim + seg_sent[sgw];
      gsim = p.dsim[o];
      vsim = p.sim[o];
    }
  }
  float lpre[PW_MAXSEG * SP / NTHR];
#pragma unroll
  for (int i = 0; i < PW_MAXSEG * SP / NTHR; ++i) {
    const int e = tid + i * NTHR, s2 = e / SP, r = e - s2 * SP;
    lpre[i] = s2 < NS ? p.lse[((size_t)b * p.n_sent + dsc[8 + s2]) * SP + r] : 0.f;
  }

#pragma unroll
  for (int i = 0; i < PW_MAXSEG * SP / NTHR; ++i) lt[tid + i * NTHR] = lpre[i] * LOG2E;
  if constexpr (AUX) {
#pragma unroll
    for (int i = 0; i < PW_MAXSEG * SP / NTHR; ++i) {
      const int e = tid + i * NTHR, s2 = e / SP, r = e - s2 * SP;
      gt[e] = (p.damean != nullptr && s2 < NS && r < p.S_eff)
                  ? p.damean[((size_t)b * p.n_sent + dsc[8 + s2]) * SP + r] / (float)dsc[24 + s2] : 0.f;
    }
  }
  if (tid < 2 * TW) {
    // per-word scalars from dsim and the forward's saved statistics (the single-tile kernel's formulas)
    float al = 0.f, be = 0.f, ka = 0.f, zi = 0.f, ga = 0.f;
    if (sgw >= 0) {
      const float Z = ws.x, cosv = ws.y, nc2 = ws.z;
      float A = __expf(vsim / p.temp3);
      if (p.agg == GLR_AGG_MEAN) A *= (float)seg_n[sgw];
      const float q = gsim * p.temp3 * p.temp2 * __expf(p.temp2 * cosv) / A;
      const float nc = sqrtf(nc2);
      const float prod = tn * nc;
      const float den = fmaxf(prod, p.eps);
      al = q / den;
      if (prod >= p.eps) { be = q * cosv / nc2; ga = q * cosv / (tn * tn); }
      ka = al * (cosv * den) - be * nc2;
      zi = Z > 0.f ? 1.f / Z : 0.f;
    }
    w4[tid] = make_float4(zi, be, al, ka);
    const size_t slot = (size_t)tile0 * TW + tid;
    p.gamma[(size_t)b * p.n_slots + slot] = ga;
    p.beta[(size_t)b * p.n_slots + slot] = be;
  }
  __syncthreads();

  GLR_STAMP2(1);
  f32x16 acc0[3], acc1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[j][q] = 0.f; acc1[j][q] = 0.f; }
  GLR_STAMP2(2);

  const int* fl = dsc + 32 + 8 * t;
  const unsigned ST0 = __builtin_amdgcn_readfirstlane(fl[0]), ST1 = __builtin_amdgcn_readfirstlane(fl[1]),
                 LA0 = __builtin_amdgcn_readfirstlane(fl[2]), LA1 = __builtin_amdgcn_readfirstlane(fl[3]);
  const unsigned STANY = ST0 | ST1, LAANY = LA0 | LA1;
  const unsigned STh = h ? ST1 : ST0, LAh = h ? LA1 : LA0;
#define GLR_SBIT(mask, k) __builtin_expect(([&] { unsigned b_ = ((mask) >> (k)) & 1u; asm volatile("" : "+s"(b_)); return b_ != 0; }()), 0)
  int sgp[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) sgp[g] = *reinterpret_cast<const int*>(wsegb + t * TW + (g >> 2) * 32 + 4 * h + 8 * (g & 3));
#define GLR_SGK(k) ((sgp[(k) >> 2] << (24 - 8 * ((k) & 3))) >> 24)
  const int rbase = wg * 32 + l31;
  const float t1l = p.temp1 * LOG2E;
  const float ok2 = (rbase + 256 < p.S_eff) ? 1.f : 0.f;          // padded regions live in block 2 only
  unsigned char* imgw = img0 + t * IMG + (4 * h) * IMP + rbase * ESZ;
  const float4* w4t = w4 + t * TW + 4 * h;

  // ================= P2 =================
  if (!GLR_SKIP(4)) {
    float lc[3] = {0.f, 0.f, 0.f};
    [[maybe_unused]] float gc[3] = {0.f, 0.f, 0.f};          // AUX: damean / n of the current run's sentence
    // AUX: gradient of the diagonal pair's attention map (attention supervision), per (word, region); at most ONE
    // workgroup per image holds the diagonal sentence
    [[maybe_unused]] const int dw0 = AUX ? misc[1] : 0, dn = (AUX && p.dattn != nullptr) ? misc[2] : 0;
    [[maybe_unused]] const int sout = p.S_eff - p.strip;
    [[maybe_unused]] const float* dmap = dn > 0 ? p.dattn + p.attn_off[p.img_offset + b] - p.strip : nullptr;
    [[maybe_unused]] float* kredt = kred + (wg * 2 + ((lane >> 4) & 1)) * (2 * TW) + t * TW + 4 * h;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      f32x16(&acc)[3] = blk == 0 ? acc0 : acc1;
      unsigned(&a1k)[3][8] = blk == 0 ? a1k0 : a1k1;
      [[maybe_unused]] float zq[4];                // reduced across lanes every four rows (interleaved DPP chains)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int k = blk * 16 + q;
        const int row = blk * 32 + (q & 3) + 8 * (q >> 2);
        if (GLR_SBIT(STANY, k)) {
          const bool mine = (STh >> k) & 1;
          const int srow = (long_pair ? 0 : max(GLR_SGK(k), 0)) * SP + rbase;
          const float* src = lt + srow;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const float l2 = src[128 * j];
            lc[j] = mine ? l2 : lc[j];
            if constexpr (AUX) {
              const float g2 = gt[srow + 128 * j];
              gc[j] = mine ? g2 : gc[j];
            }
          }
        }
        const float4 w = w4t[row];
        [[maybe_unused]] float ge[3] = {gc[0], gc[1], ok2 * gc[2]};
        if constexpr (AUX) {
          if (__builtin_expect(dn > 0, 0)) {
            const int wd = t * TW + row + 4 * h - dw0;
            if (wd >= 0 && wd < dn) {
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                const int region = rbase + 128 * j;
                if (region >= p.strip && region < p.S_eff) ge[j] += dmap[(size_t)wd * sout + region];
              }
            }
          }
        }
        [[maybe_unused]] float zacc = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const h2 hp = __builtin_bit_cast(h2, a1k[j][q >> 1]);
          const float a1 = (float)((q & 1) ? hp.y : hp.x);            // <= 1: the forward clamps what it hands over
          const float sc = (lc[j] + __builtin_amdgcn_logf(fmaxf(a1, 5.9604645e-8f))) * LN2;     // s = lse + log a1
          const float a2 = __builtin_amdgcn_exp2f(t1l * a1) * w.x;
          O::from_f32(imgw + row * IMP + 128 * j * ESZ, w.y * a2);
          if constexpr (AUX) {
            acc[j][q] = __builtin_fmaf(-w.z, sc, -ge[j]);       // da2 = (alpha s - beta u) + g
            zacc = __builtin_fmaf(a2, ge[j], zacc);             // kappa gains sum_r a2 g (softmax-over-regions backward)
          } else {
            acc[j][q] = -w.z * sc;
          }
          asm volatile("" : "+v"(acc[j][q]));                   // computed HERE (not sunk to its use behind the barrier)
        }
        if constexpr (AUX) {
          zq[q & 3] = zacc;
          if ((q & 3) == 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float z = row_sum16(zq[i]);
              if ((lane & 15) == 15) kredt[blk * 32 + i + 8 * (q >> 2)] = z;
            }
          }
        }
      }
    }
  }
  __syncthreads();                              // images complete; lt is dead: the P3 ring takes its place
  if constexpr (AUX) {
    if (tid < 2 * TW) {                         // read by pass A behind the barriers of the P3 stream
      float kg = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) kg += kred[k * (2 * TW) + tid];
      w4[tid].w += kg;
    }
  }
  GLR_STAMP2(3);

  // ================= P3: acc += (beta a2) . G^T =================
  if (!GLR_SKIP(8))
  stream_gemm<O, true, 2, 2>(acc0, acc1, 0, 32 * IMP, ring3, SP * CB, nullptr, 0, gram_b, rowbytes2, SP,
                            (int)(rowbytes2 / CB), img0 + t * IMG, IMP, wave, lane, 0, wg, NRB, TW);
  GLR_STAMP2(4);

  if (p.baout != nullptr && !GLR_SKIP(128)) {
    // the operand image beta a2 itself is the third output
    for (int i = tid; i < 2 * TW * PPR; i += NTHR) {
      const int row = i / PPR, pc = i - row * PPR;
      const uint4 v = *reinterpret_cast<const uint4*>(img0 + (row >> 6) * IMG + (row & 63) * IMP + pc * 16);
      st_stream16(p.baout + ((size_t)b * p.n_slots + (size_t)tile0 * TW + row) * (SP * ESZ) + pc * 16, v, GLR_SKIP(256));
    }
    __syncthreads();
  }

  // ================= A: da1, run sums of a1 da1, a2 image =================
  // (opaque copies: the compiler otherwise keeps P2's unpacked fp32 a1 alive - spilled - for this pass)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) { asm volatile("" : "+v"(a1k0[j][i])); asm volatile("" : "+v"(a1k1[j][i])); }
  GLR_STAMP2(5);
  const int nrow = long_pair ? 2 : NS;
  {
    float* tz = rh + h * HT + rbase;
    for (int s2 = 0; s2 < nrow; ++s2) {
      if ((long_pair ? s2 : (seg_w0[s2] >> 6)) != t) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) tz[s2 * SP + 128 * j] = 0.f;
    }
  }
  if (!GLR_SKIP(32)) {
    float rs[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
      const unsigned(&a1k)[3][8] = k < 16 ? a1k0 : a1k1;
      const int q = k & 15;
      const int row = (k >> 4) * 32 + (q & 3) + 8 * (q >> 2);
      const float4 w = w4t[row];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const h2 hp = __builtin_bit_cast(h2, a1k[j][q >> 1]);
        const float a1 = (float)((q & 1) ? hp.y : hp.x);
        const float a2 = __builtin_amdgcn_exp2f(t1l * a1) * w.x;
        const float da1 = p.temp1 * a2 * (-acc[j][q] - w.w);
        const float pr = a1 * da1;
        rs[j] += pr;
        acc[j][q] = __builtin_fmaf(w.z, a2, pr);
        asm volatile("" : "+v"(acc[j][q]));
        O::from_f32(imgw + row * IMP + 128 * j * ESZ, j == 2 ? ok2 * a2 : a2);
      }
      if (GLR_SBIT(LAANY, k)) {
        const bool mine = (LAh >> k) & 1;
        if (mine) {
          float* dst = rh + h * HT + (long_pair ? t : GLR_SGK(k)) * SP + rbase;
#pragma unroll
          for (int j = 0; j < 3; ++j) dst[128 * j] = rs[j];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[j] = mine ? 0.f : rs[j];
      }
    }
  }
  __syncthreads();                              // a2 images and the run-sum tables (both tiles) are complete
  GLR_STAMP2(6);
  if (!GLR_SKIP(128))
  for (int i = tid; i < 2 * TW * PPR; i += NTHR) {
    const int row = i / PPR, pc = i - row * PPR;
    const uint4 v = *reinterpret_cast<const uint4*>(img0 + (row >> 6) * IMG + (row & 63) * IMP + pc * 16);
    st_stream16(p.aout + ((size_t)b * p.n_slots + (size_t)tile0 * TW + row) * (SP * ESZ) + pc * 16, v, GLR_SKIP(256));
  }

  // ================= B: X = acc - a1 rho (registers), then through the image to xout =================
  // (opaque copies: the compiler otherwise keeps pass A's unpacked fp32 a1 alive - spilled - for this pass)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) { asm volatile("" : "+v"(a1k0[j][i])); asm volatile("" : "+v"(a1k1[j][i])); }
  if (!GLR_SKIP(64)) {
    const float* r1 = (long_pair ? rh + SP : zero) + rbase;      // second row: the other tile's (spanning sentence) or zeros
    const int HT2 = long_pair ? HT : 0;
    float rc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
      const unsigned(&a1k)[3][8] = k < 16 ? a1k0 : a1k1;
      const int q = k & 15;
      if (GLR_SBIT(STANY, k)) {
        const bool mine = (STh >> k) & 1;
        const float* r0 = rh + (long_pair ? 0 : max(GLR_SGK(k), 0)) * SP + rbase;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float rho = (r0[128 * j] + r0[HT + 128 * j]) + (r1[128 * j] + r1[HT2 + 128 * j]);
          rc[j] = mine ? rho : rc[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const h2 hp = __builtin_bit_cast(h2, a1k[j][q >> 1]);
        const float a1 = (float)((q & 1) ? hp.y : hp.x);
        const float x = __builtin_fmaf(-a1, rc[j], acc[j][q]);
        acc[j][q] = j == 2 ? ok2 * x : x;
        asm volatile("" : "+v"(acc[j][q]));
      }
    }
  }
#undef GLR_SBIT
#undef GLR_SGK
  __syncthreads();                              // every thread has read its a2 rows out of the image
  GLR_STAMP2(7);
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const f32x16(&acc)[3] = k < 16 ? acc0 : acc1;
    const int q = k & 15;
    const int row = (k >> 4) * 32 + (q & 3) + 8 * (q >> 2);
#pragma unroll
    for (int j = 0; j < 3; ++j) O::from_f32(imgw + row * IMP + 128 * j * ESZ, acc[j][q]);
  }
  __syncthreads();
  GLR_STAMP2(8);
  if (!GLR_SKIP(128))
  for (int i = tid; i < 2 * TW * PPR; i += NTHR) {
    const int row = i / PPR, pc = i - row * PPR;
    const uint4 v = *reinterpret_cast<const uint4*>(img0 + (row >> 6) * IMG + (row & 63) * IMP + pc * 16);
    st_stream16(p.xout + (((size_t)tile0 * TW + row) * p.B_img + b) * (SP * ESZ) + pc * 16, v, GLR_SKIP(256));
  }
  GLR_STAMP2(9);
}

#ifdef GLR_STAMPS
unsigned long long* g_stamps = nullptr;
unsigned long long* g_stamps2 = nullptr;
#endif

int carve(LaParams& p, int op_dtype, int S_pad) {
  const int esz = op_dtype == GLR_F32 ? 4 : 2;
  const int ring1 = NBUF * (p.tw + S_pad) * CHB;   // P1 ring
  const int ring2 = NBUF * S_pad * CHB;            // P3 ring (must not overlap the image)
  const int sc_bytes = p.tw * GLR_MAX_SPAD * 4;    // score tile / rho (alias the ring, dead when it runs)
  const int img_bytes = p.tw * (GLR_MAX_SPAD * esz + 16);
  p.off_img = max(ring2, sc_bytes);                // the P1 ring may run over the image: it is dead then
  p.off_small = max(p.off_img + img_bytes, ring1);
  return p.off_small + 12288;
}

// pair kernel: [0, 2*IMG) images (earlier: P1 ring) | statistics tables, then the 2-deep P3 ring | small
int carve_pair(LaParams& p, int op_dtype, int S_pad) {
  const int esz = op_dtype == GLR_F32 ? 4 : 2;
  const int img_bytes = TW * (GLR_MAX_SPAD * esz + 16);
  const int tab_bytes = 4 * PW_MAXSEG * S_pad * 4;            // maxima + sums, one table per lane half
  const int ring3 = 2 * S_pad * CHB;
  const int ring1 = NBUF * (2 * p.tw + S_pad) * CHB;
  p.off_img = 2 * img_bytes;                       // tables / P3 ring
  p.off_small = max(p.off_img + max(tab_bytes, ring3), ring1);
  return p.off_small + 12288;
}

template <bool BWD>
int launch(LaParams& p, int op_dtype, void* stream) {
  const int lds = carve(p, op_dtype, p.S_pad);
  if (lds > 160 * 1024) return GLR_EINVAL;
  const int grid = p.pair_only ? p.B_img : ((p.B_img + 7) / 8) * 8 * p.n_items;
  if (grid <= 0) return GLR_OK;
  hipStream_t st = (hipStream_t)stream;
#define GLR_LAUNCH_K1(OP, FULL)                                                                                      \
  do {                                                                                                               \
    if (BWD && (p.damean != nullptr || p.dattn != nullptr)) {                                                        \
      static GlrLdsAttr la_;                                                                                         \
      if (glr_ensure_lds(la_, (const void*)k_local_attn<OP, BWD, FULL, BWD>, lds) != GLR_OK) return GLR_ELAUNCH;     \
      hipLaunchKernelGGL((k_local_attn<OP, BWD, FULL, BWD>), dim3(grid), dim3(NTHR), lds, st, p);                     \
    } else {                                                                                                         \
      static GlrLdsAttr la_;                                                                                         \
      if (glr_ensure_lds(la_, (const void*)k_local_attn<OP, BWD, FULL, false>, lds) != GLR_OK) return GLR_ELAUNCH;   \
      hipLaunchKernelGGL((k_local_attn<OP, BWD, FULL, false>), dim3(grid), dim3(NTHR), lds, st, p);                   \
    }                                                                                                                \
  } while (0)
  const bool full = p.S_pad == GLR_MAX_SPAD;
  if (op_dtype == GLR_BF16) {
    if (full) GLR_LAUNCH_K1(OpBF16, true); else GLR_LAUNCH_K1(OpBF16, false);
  } else {
    if (full) GLR_LAUNCH_K1(OpF32, true); else GLR_LAUNCH_K1(OpF32, false);
  }
#undef GLR_LAUNCH_K1
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

int launch_pair(LaParams& p, int op_dtype, void* stream) {
  if (op_dtype != GLR_BF16) return GLR_EINVAL;      // the fp32 mode (32-word tiles) is never paired
  if (p.S_pad != GLR_MAX_SPAD) return GLR_EINVAL;   // the pair kernels are built for the 384-region shape only
  const int lds = carve_pair(p, op_dtype, p.S_pad);
  if (lds > 160 * 1024) return GLR_EINVAL;
  // the pair kernel needs the planner's row flags and a spare padded region for the ones row of the Gram operand
  if (p.pair_desc == nullptr || p.S_eff >= p.S_pad) return GLR_EINVAL;
  const int grid = glr_k1_pair_grid(p, 1);
  static GlrLdsAttr la_pw;
  if (glr_ensure_lds(la_pw, (const void*)k_local_attn_pw<OpBF16>, lds) != GLR_OK) return GLR_ELAUNCH;
  hipLaunchKernelGGL((k_local_attn_pw<OpBF16>), dim3(grid), dim3(NTHR), lds, (hipStream_t)stream, p);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

int launch_pair_bwd(LaParams& p, int op_dtype, void* stream) {
  if (op_dtype != GLR_BF16 || p.S_pad != GLR_MAX_SPAD) return GLR_EINVAL;
  if (p.a1buf == nullptr) return GLR_EINVAL;        // the scores come from the a1 the forward handed over
  const int lds = carve_pair(p, op_dtype, p.S_pad);
  // the kernel's lse table (LT_OFF) lies in front of the small area
  if (lds > 160 * 1024 || NBUF * (2 * TW + p.S_pad) * CHB + PW_MAXSEG * p.S_pad * 4 > p.off_small) return GLR_EINVAL;
  if (p.pair_desc == nullptr || p.S_eff >= p.S_pad) return GLR_EINVAL;
  const int grid = glr_k1_pair_grid(p, 1);
  if (p.damean != nullptr || p.dattn != nullptr) {
    static GlrLdsAttr la_b2;
    if (glr_ensure_lds(la_b2, (const void*)k_local_attn_pw_bwd<OpBF16, true>, lds) != GLR_OK) return GLR_ELAUNCH;
    hipLaunchKernelGGL((k_local_attn_pw_bwd<OpBF16, true>), dim3(grid), dim3(NTHR), lds, (hipStream_t)stream, p);
  } else {
    static GlrLdsAttr la_b1;
    if (glr_ensure_lds(la_b1, (const void*)k_local_attn_pw_bwd<OpBF16, false>, lds) != GLR_OK) return GLR_ELAUNCH;
    hipLaunchKernelGGL((k_local_attn_pw_bwd<OpBF16, false>), dim3(grid), dim3(NTHR), lds, (hipStream_t)stream, p);
  }
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

// Everything the two entry points share: argument checks, the plan header (host) -> counts and device pointers.
int fill_common(LaParams& p, const void* vt, const void* gram, const void* tp, const float* tnorm, const int32_t* plan,
                const int32_t* plan_dev, int B_img, int D, int S_eff, float temp1, float temp2, float temp3, int agg,
                float eps, int op_dtype) {
  if (!vt || !gram || !tp || !tnorm || !plan || !plan_dev) return GLR_EINVAL;
  if (op_dtype != GLR_F32 && op_dtype != GLR_BF16) return GLR_EDTYPE;
  const int n_sent = plan[GLR_PLAN_N_SENT], n_tiles = plan[GLR_PLAN_N_TILES], n_ints = plan[GLR_PLAN_N_INTS];
  const int n_pair = plan[GLR_PLAN_N_PAIR];
  if (n_tiles <= 0 || n_sent <= 0 || B_img <= 0 || S_eff <= 0 || D <= 0 || D % 64 != 0) return GLR_EINVAL;
  if (plan[GLR_PLAN_N_ORDER] < 0 || plan[GLR_PLAN_N_SINGLE] < 0 || n_pair < 0 || plan[GLR_PLAN_N_LONG_PAIR] < 0 ||
      plan[GLR_PLAN_N_LONG_PAIR] > n_pair || plan[GLR_PLAN_CAPACITY] != glr_tile_capacity(op_dtype))
    return GLR_EINVAL;
  const int len[8] = {n_sent, n_sent, n_tiles + 1, plan[GLR_PLAN_N_ORDER], n_tiles, plan[GLR_PLAN_N_SINGLE], n_pair, 64 * n_pair};
  for (int a = 0; a < 8; ++a) {
    const int off = plan[GLR_PLAN_OFF_CAP_LENS + a];
    if (off < GLR_PLAN_HEADER || (long long)off + len[a] > n_ints) return GLR_EINVAL;
  }
  const int S_pad = glr_region_pad(S_eff);
  if (S_pad > GLR_MAX_SPAD) return GLR_EINVAL;
  if (agg < 0 || agg > 2) return GLR_EINVAL;
  p.vt = (const unsigned char*)vt; p.gram = (const unsigned char*)gram; p.tp = (const unsigned char*)tp;
  p.tnorm = tnorm;
  p.cap_lens = plan_dev + plan[GLR_PLAN_OFF_CAP_LENS]; p.sent_slot0 = plan_dev + plan[GLR_PLAN_OFF_SENT_SLOT0];
  p.tile_first = plan_dev + plan[GLR_PLAN_OFF_TILE_FIRST]; p.order = plan_dev + plan[GLR_PLAN_OFF_ORDER];
  p.tile_nsub = plan_dev + plan[GLR_PLAN_OFF_TILE_NSUB];
  p.item_tile = nullptr; p.n_items = 0; p.amean = nullptr; p.damean = nullptr; p.dattn = nullptr; p.pair_desc = nullptr; p.a1buf = nullptr; p.a1_items = 0; p.a1_base = 0; p.n_tiles = n_tiles; p.n_sent = n_sent;
  p.n_slots = n_tiles * TW; p.B_img = B_img;
  p.D = D; p.S_eff = S_eff; p.S_pad = S_pad; p.temp1 = temp1; p.temp2 = temp2; p.temp3 = temp3; p.agg = agg;
  p.eps = eps;
  p.tw = glr_tile_capacity(op_dtype);
  p.attn = nullptr; p.attn_off = nullptr; p.strip = 0; p.pair_only = 0; p.img_offset = 0;
  p.dsim = nullptr; p.xout = nullptr; p.aout = nullptr; p.gamma = nullptr; p.beta = nullptr; p.baout = nullptr;
  p.lse = nullptr; p.wstat = nullptr; p.sim = nullptr; p.ld_sim = 0;
#ifdef GLR_STAMPS
  p.stamps = g_stamps;
  p.stamps2 = g_stamps2;
#endif
  return GLR_OK;
}

}  // namespace

extern "C" int glr_local_attn_fwd(const void* vt, const void* gram, const void* tp, const float* tnorm,
                                  const int32_t* plan, const int32_t* plan_dev, int B_img, int D, int S_eff, float temp1,
                                  float temp2, float temp3, int agg, float eps, float* sim, int ld_sim, float* lse,
                                  float* wstat, float* attn, const int64_t* attn_off, int strip, int pair_only,
                                  int img_offset, float* amean, void* a1buf, int op_dtype, void* stream) {
  LaParams p;
  int rc = fill_common(p, vt, gram, tp, tnorm, plan, plan_dev, B_img, D, S_eff, temp1, temp2, temp3, agg, eps, op_dtype);
  if (rc != GLR_OK) return rc;
  const int n_single = plan[GLR_PLAN_N_SINGLE], n_pair = plan[GLR_PLAN_N_PAIR], n_long_pair = plan[GLR_PLAN_N_LONG_PAIR];
  const int32_t* pair_tile = plan_dev + plan[GLR_PLAN_OFF_PAIR_TILE];
  const int32_t* pair_desc = plan_dev + plan[GLR_PLAN_OFF_PAIR_DESC];
  if (!sim || (attn && !attn_off)) return GLR_EINVAL;
  if (img_offset < 0) return GLR_EINVAL;          // sent_slot0 / attn_off are indexed with img_offset + b
  if (pair_only && img_offset + B_img > p.n_sent) return GLR_EINVAL;
  if (!pair_only && n_single + n_pair == 0) return GLR_EINVAL;
  if (amean && pair_only) return GLR_EINVAL;
  p.sim = sim; p.ld_sim = ld_sim; p.lse = lse; p.wstat = wstat; p.attn = attn; p.amean = amean;
  p.attn_off = (const long long*)attn_off; p.strip = strip; p.pair_only = pair_only; p.img_offset = img_offset;
  if (pair_only || n_single > 0) {
    p.item_tile = plan_dev + plan[GLR_PLAN_OFF_SINGLE_TILE]; p.n_items = n_single;
    rc = launch<false>(p, op_dtype, stream);
    if (rc != GLR_OK) return rc;
  }
  if (!pair_only && n_pair > 0) {
    // The pairs of one 65..128-word sentence (a prefix of the pair list: the planner puts multi-tile sentences first) run
    // the 8-wave pair kernel; the ordinary pairs (two whole tiles) run one 4-wave workgroup per tile, two per CU
    // (glr_local_attn_t1.hip).  GLR_K1_T1=0 sends every pair to the pair kernel (A/B switch of tools/ and tests).
    static const bool use_t1 = [] { const char* e = getenv("GLR_K1_T1"); return !(e && e[0] == '0'); }();
    const int n_pw = (use_t1 && D % 128 == 0 && D >= 256) ? n_long_pair : n_pair;
    p.a1buf = (unsigned*)a1buf; p.a1_items = n_pair;
    if (n_pw > 0) {
      p.item_tile = pair_tile; p.n_items = n_pw; p.pair_desc = pair_desc; p.a1_base = 0;
      rc = launch_pair(p, op_dtype, stream);
      if (rc != GLR_OK) return rc;
    }
    if (n_pair > n_pw) {
      p.item_tile = pair_tile + n_pw; p.n_items = n_pair - n_pw; p.pair_desc = pair_desc + (size_t)64 * n_pw; p.a1_base = n_pw;
      rc = glr_k1_launch_tiles(p, op_dtype, stream);
    }
  }
  return rc;
}

extern "C" int glr_local_attn_bwd(const void* vt, const void* gram, const void* tp, const float* tnorm,
                                  const int32_t* plan, const int32_t* plan_dev, int B_img, int D, int S_eff, float temp1,
                                  float temp2, float temp3, int agg, float eps, const float* sim, const float* dsim,
                                  int ld_sim, const float* lse, const float* wstat, const float* damean,
                                  const float* dattn, const int64_t* attn_off, int strip, int img_offset, void* xout,
                                  void* aout, void* baout, float* gamma, float* beta, const void* a1buf, int op_dtype,
                                  void* stream) {
  LaParams p;
  int rc = fill_common(p, vt, gram, tp, tnorm, plan, plan_dev, B_img, D, S_eff, temp1, temp2, temp3, agg, eps, op_dtype);
  if (rc != GLR_OK) return rc;
  const int n_single = plan[GLR_PLAN_N_SINGLE], n_pair = plan[GLR_PLAN_N_PAIR];
  if (!sim || !dsim || !lse || !wstat || !xout || !aout || !gamma || !beta) return GLR_EINVAL;
  if (n_single + n_pair == 0) return GLR_EINVAL;
  if (agg == GLR_AGG_MAX) return GLR_EINVAL;      // max aggregation is inference-only (gloria_model.py:199)
  p.sim = const_cast<float*>(sim); p.dsim = dsim; p.ld_sim = ld_sim; p.lse = const_cast<float*>(lse);
  p.wstat = const_cast<float*>(wstat); p.xout = (unsigned char*)xout; p.aout = (unsigned char*)aout;
  p.baout = (unsigned char*)baout;
  if (dattn && !attn_off) return GLR_EINVAL;
  if (img_offset < 0 || img_offset + B_img > p.n_sent) return GLR_EINVAL;
  p.gamma = gamma; p.beta = beta; p.damean = damean;
  p.dattn = dattn; p.attn_off = (const long long*)attn_off; p.strip = strip; p.img_offset = img_offset;
  if (n_single > 0) {
    p.item_tile = plan_dev + plan[GLR_PLAN_OFF_SINGLE_TILE]; p.n_items = n_single;
    rc = launch<true>(p, op_dtype, stream);
    if (rc != GLR_OK) return rc;
  }
  if (n_pair > 0) {
    p.item_tile = plan_dev + plan[GLR_PLAN_OFF_PAIR_TILE]; p.n_items = n_pair;
    p.pair_desc = plan_dev + plan[GLR_PLAN_OFF_PAIR_DESC]; p.a1buf = (unsigned*)const_cast<void*>(a1buf);
    p.a1_items = n_pair; p.a1_base = 0;
    rc = launch_pair_bwd(p, op_dtype, stream);
  }
  return rc;
}

#ifdef GLR_STAMPS
// diagnostic build only: device buffer of [grid][12] u64 receiving s_memtime stamps of every K1 launch
extern "C" void glr_debug_set_stamps(void* buf) { g_stamps = (unsigned long long*)buf; }
extern "C" void glr_debug_set_stamps_pair(void* buf) { g_stamps2 = (unsigned long long*)buf; }
extern "C" void glr_debug_set_wave_stamps(void* buf) {
  unsigned long long* v = (unsigned long long*)buf;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_stamps), &v, sizeof(v));
}
#endif
